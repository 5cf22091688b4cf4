// EXTENSION: the causal multi-query paged scan -- attention for the positions of a prompt, which the decode scans (one
// query per row, one pass over the row's pages) cannot give without reading a row's pages once per position.
//   A SEGMENT is (row b, first position p, count n): its query j is position t = p + j of row b, 0 <= t < n_sequence.
//   Query t attends slot s of row b iff s <= t and (no window, or s > t - window, or s < n_sink); one softmax per head over
//   q_h . K_h / sqrtf(head_dim); query head h reads K/V head h / g (gqa_kv_unit).  That is what the decode scans
//   (scan_item_body.hpp, heads_item_body.hpp) compute for a row of length t + 1.
// One 256-thread workgroup per (segment, block of TQ consecutive queries).  It streams the pages the block attends ONCE, a
// wave owning whole pages, with the decode scans' buffer-resource 16-byte lane loads and rolling register prefetch; every
// K unit a lane loads is dotted with its TQ query vectors held in registers, every V unit accumulated into TQ accumulators:
// the K/V bytes per query fall by TQ.  Online-softmax state is kept per query -- per wave with one head (the transposing
// butterfly of wave_reduce16, a slot's probability broadcast through an SGPR), per lane with several (lane groups and the
// DPP butterfly of heads_item_body.hpp).  The four waves are merged through LDS in wave order, one query at a time.  There
// is no split along the key axis: parallelism comes from segments x query blocks, so there is no workspace, no arrival
// counter and no second launch.
// The mask is per (query, slot); a masked slot's data is never multiplied, not even by zero (slots above a query's position
// hold unwritten bytes).  The pages that are dead for EVERY query of the block -- those wholly between the sinks and the
// window of the block's first query -- are never visited and their table entries never read: the waves walk the virtual row
// of sink pages + window pages (sink_page, scan_item_body.hpp), a wave-uniform map.
// Device values never fault: a segment whose row, positions or offset fall outside (n_batch, n_sequence, n_q) is skipped
// whole, a null page reads as zeros.  An `out` row that belongs to no query is never written.
//
//   grid = n_seg * ceil(max_count / TQ) workgroups (surplus ones exit), 256 threads, no dynamic LDS
#pragma once

#include "heads_item_body.hpp"
#include "launch_count.hpp"

namespace mli {

#define MLI_PROMPT_SINK_LOGITS 0
#define MLI_PROMPT_SOFTCAP 0
#include "prompt_scan_body.hpp"   // prompt_scan_kernel
#undef MLI_PROMPT_SOFTCAP
#define MLI_PROMPT_SOFTCAP 1
#include "prompt_scan_body.hpp"   // prompt_softcap_scan_kernel (EXTENSION, attention_softcap.hpp)
#undef MLI_PROMPT_SOFTCAP
#undef MLI_PROMPT_SINK_LOGITS
#define MLI_PROMPT_SOFTCAP 0
#define MLI_PROMPT_SINK_LOGITS 1
#include "prompt_scan_body.hpp"   // prompt_sink_logits_scan_kernel (EXTENSION, attention_sink_logits.hpp)
#undef MLI_PROMPT_SINK_LOGITS
#undef MLI_PROMPT_SOFTCAP

// The launch with sink logits for an accepted shape with H > 1 (prompt_scan_shape_ok), sink_logits non-null: launch_prompt_scan's
// grid with the same TQ (prompt_scan_tq), counted as "scan_prompt_sink_logits".
template <class E>
int launch_prompt_sink_logits_scan(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                   const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                                   int B, int S, int D, int H, int Hkv, int lg, int window, int n_sink, const float* sink_logits,
                                   hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const auto go = [&](auto NJ) {
        constexpr int TQ = prompt_scan_tq(E::EPL, NJ(), true);
        const int nb = ceil_div_i(max_count, TQ);
        if (!prompt_scan_grid_ok(n_seg, max_count, TQ)) return (int)MLI_ERR_BAD_ARG;   // (the entry points refuse it first)
        count_launch(kLfScanPromptSinkLogits);
        hipLaunchKernelGGL((prompt_sink_logits_scan_kernel<E, NJ(), TQ>), dim3((unsigned)(n_seg * nb)), dim3(kFuThreads), 0, st,
                           q, page_table, seg_row, seg_first, seg_count, seg_offset, out, nb, n_q, B, S, D, lg, H / Hkv, window,
                           n_sink, sink_logits);
        return launch_status();
    };
    using std::integral_constant;
    return nj == 1 ? go(integral_constant<int, 1>{}) : go(integral_constant<int, 2>{});
}

// The capped launch for an accepted shape with H > 1 (prompt_scan_shape_ok), cap > 0 finite: launch_prompt_scan's grid with
// the same TQ (prompt_scan_tq: the capped kernels compile without scratch at it), counted as "scan_prompt_softcap".
template <class E>
int launch_prompt_softcap_scan(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                               const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q, int B,
                               int S, int D, int H, int Hkv, int lg, int window, int n_sink, float cap, hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const auto go = [&](auto NJ) {
        constexpr int TQ = prompt_scan_tq(E::EPL, NJ(), true);
        const int nb = ceil_div_i(max_count, TQ);
        if (!prompt_scan_grid_ok(n_seg, max_count, TQ)) return (int)MLI_ERR_BAD_ARG;   // (the entry points refuse it first)
        count_launch(kLfScanPromptSoftcap);
        hipLaunchKernelGGL((prompt_softcap_scan_kernel<E, NJ(), TQ>), dim3((unsigned)(n_seg * nb)), dim3(kFuThreads), 0, st, q,
                           page_table, seg_row, seg_first, seg_count, seg_offset, out, nb, n_q, B, S, D, lg, H / Hkv, window,
                           n_sink, cap);
        return launch_status();
    };
    using std::integral_constant;
    return nj == 1 ? go(integral_constant<int, 1>{}) : go(integral_constant<int, 2>{});
}

// The launch for an accepted shape (prompt_scan_shape_ok): H heads on Hkv K/V heads, lg = heads_lanes_log2 where H > 1;
// window 0 = none.  n_seg >= 1, max_count >= 1.
template <class E>
int launch_prompt_scan(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                       const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q, int B, int S,
                       int D, int H, int Hkv, int lg, int window, int n_sink, hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const auto go = [&](auto NJ, auto HEADS) {
        constexpr int TQ = prompt_scan_tq(E::EPL, NJ(), HEADS());
        const int nb = ceil_div_i(max_count, TQ);
        if (!prompt_scan_grid_ok(n_seg, max_count, TQ)) return (int)MLI_ERR_BAD_ARG;   // (the entry points refuse it first)
        count_launch(kLfScanPrompt);
        hipLaunchKernelGGL((prompt_scan_kernel<E, NJ(), TQ, HEADS()>), dim3((unsigned)(n_seg * nb)), dim3(kFuThreads), 0, st, q,
                           page_table, seg_row, seg_first, seg_count, seg_offset, out, nb, n_q, B, S, D, lg, H / Hkv, window,
                           n_sink);
        return launch_status();
    };
    using std::integral_constant;
    if (H > 1) return nj == 1 ? go(integral_constant<int, 1>{}, std::true_type{}) : go(integral_constant<int, 2>{}, std::true_type{});
    return nj == 1 ? go(integral_constant<int, 1>{}, std::false_type{}) : go(integral_constant<int, 2>{}, std::false_type{});
}

}  // namespace mli
