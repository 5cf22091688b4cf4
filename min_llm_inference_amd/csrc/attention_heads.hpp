// EXTENSION: multi-head attention for the paged decode scan (lean form, chunked grid, in-kernel merge).
//   n_heads = H, head_dim = hd = emb_dim / H; head h owns columns [h * hd, (h + 1) * hd) of q_output and of the K and V
//   segments of every page slot; one softmax per head over q_h . K_h / sqrtf(hd).
// The scan reads exactly the bytes the single-head scan reads, with the same grid, prefetch and hand-off; the workgroup
// body (heads_item_body.hpp) keeps its softmax state per head.  H == 1 never comes here: launch_lean_scan (compose.hip)
// takes it to the single-head scans.
// Every form of the multi-head scan is this file's one kernel template with the body's compile-time switches:
//   WIN   sliding window, window = W, 1 <= W < n_sequence: row b attends slots [lo, L), L = min(lengths[b], n_sequence),
//         lo = max(0, L - W).  The row starts at its first live page and the grid, the item size and the workspace traffic
//         follow the span the window leaves (attention_window.hpp has the single-head form and the details).
//   SINK  (with WIN) n_sink = K >= 1, K + W < n_sequence: the row attends its first K tokens as well, as a virtual row of
//         sink pages and window pages.
//   GQA   grouped-query attention, n_kv_heads = Hkv < H, H % Hkv == 0, g = H / Hkv (any integer): query head h attends K/V
//         head h / g, which owns columns [(h / g) * hd, (h / g + 1) * hd) of the K and the V segment of every page slot;
//         columns >= Dkv = Hkv * hd of those segments are never read.  That is multi-head attention with H heads on pages
//         whose K / V column block h is a copy of block h / g.  What the switch changes is the 16-byte unit a lane loads
//         (gqa_kv_unit, scan_plan.hpp): the lanes of the g query heads of a group issue the same addresses inside one load
//         instruction, so the bytes fetched from memory fall by g while the load instructions do not.  Grid, item size,
//         workspace, LDS, merge and arrival counters are those of H heads; the cache policy of the K / V loads is judged by
//         the Dkv columns actually read.
// The merge, the arrival counters and the workspace layout are the same in every form.  fp32 and bf16 pages, each compiled
// in a file of its own (attention_heads.hip, attention_heads_bf16.hip: 24 kernels each) so that neither is the longest step
// of a build.
//
//   grid = (B, items of the span + 1) rows fast, 256 threads, a wave owns whole pages; one launch, no combine kernel
#pragma once

#include "heads_item_body.hpp"
#include "scan_launch.hpp"
#include "scan_row_order.hpp"

namespace mli {

// window, n_sink: 0 where the switch is off; gq = H / Hkv, 1 without GQA
template <class E, int NJ, bool NT, bool WIN, bool SINK, bool GQA>
__global__ __launch_bounds__(kFuThreads, 2) void heads_decode_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window, int n_sink, int gq) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // rows rotated by the item index: the items of one row spread over the XCDs (fused_decode_scan_kernel)
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<WIN, SINK>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window, n_sink);
    // 8 token slots per batch for rows of one lane load, 4 for rows of two; three batches in flight, except bf16 rows of
    // two lane loads: their 16 + 16 floats of q and output and 32 probabilities leave room for two live batches beside the
    // one being consumed without spilling
    constexpr int PD = (NJ == 2 && E::EPL == 8) ? 2 : 3;
    heads_scan_item<E, NJ, NT, NJ == 1 ? 8 : 4, PD, WIN, SINK, GQA>(q, page_table, lengths, out, ml, partial, S, D, lg, H, ct,
                                                                    nchunk_max, direct, arrivals, b, c, c == 0, smem_raw,
                                                                    window, n_sink, gq);
}

// EXTENSION (attention_alibi.hpp): the same kernel with the body's ALIBI switch on and the slopes as one more argument -- a
// kernel of its own name, so that the kernels above keep their symbols and their device code.
template <class E, int NJ, bool NT, bool WIN, bool SINK, bool GQA>
__global__ __launch_bounds__(kFuThreads, 2) void heads_alibi_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window, int n_sink, int gq, const float* __restrict__ slopes) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<WIN, SINK>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window, n_sink);
    constexpr int PD = (NJ == 2 && E::EPL == 8) ? 2 : 3;   // as heads_decode_scan_kernel
    heads_scan_item<E, NJ, NT, NJ == 1 ? 8 : 4, PD, WIN, SINK, GQA, true>(q, page_table, lengths, out, ml, partial, S, D, lg, H,
                                                                          ct, nchunk_max, direct, arrivals, b, c, c == 0,
                                                                          smem_raw, window, n_sink, gq, slopes);
}

// EXTENSION (attention_softcap.hpp): the same kernel with the body's SOFTCAP switch on and the cap as one more argument, again
// under a name of its own.
template <class E, int NJ, bool NT, bool WIN, bool SINK, bool GQA>
__global__ __launch_bounds__(kFuThreads, 2) void heads_softcap_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window, int n_sink, int gq, float cap) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<WIN, SINK>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window, n_sink);
    constexpr int PD = (NJ == 2 && E::EPL == 8) ? 2 : 3;   // as heads_decode_scan_kernel
    heads_scan_item<E, NJ, NT, NJ == 1 ? 8 : 4, PD, WIN, SINK, GQA, false, true>(q, page_table, lengths, out, ml, partial, S, D, lg,
                                                                                 H, ct, nchunk_max, direct, arrivals, b, c, c == 0,
                                                                                 smem_raw, window, n_sink, gq, nullptr, cap);
}

// EXTENSION (attention_sink_logits.hpp): the same kernel with the body's SINKLOGIT switch on and the sink logits (n_heads floats
// in device memory) as one more argument, again under a name of its own.
template <class E, int NJ, bool NT, bool WIN, bool SINK, bool GQA>
__global__ __launch_bounds__(kFuThreads, 2) void heads_sink_logits_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window, int n_sink, int gq, const float* __restrict__ sink_logits) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<WIN, SINK>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window, n_sink);
    constexpr int PD = (NJ == 2 && E::EPL == 8) ? 2 : 3;   // as heads_decode_scan_kernel
    heads_scan_item<E, NJ, NT, NJ == 1 ? 8 : 4, PD, WIN, SINK, GQA, false, false, true>(
        q, page_table, lengths, out, ml, partial, S, D, lg, H, ct, nchunk_max, direct, arrivals, b, c, c == 0, smem_raw, window,
        n_sink, gq, nullptr, 0.f, sink_logits);
}

// Grid, item size, workspace and LDS: scan_plan.hpp, at the span the form leaves and the read width Dkv (D without GQA).
// ALIBI (slopes: n_heads floats in device memory): heads_alibi_scan_kernel on the same plan, counted in a family of its own.
// SOFTCAP (cap: a finite host value > 0): heads_softcap_scan_kernel likewise ("scan_heads_softcap").
// SINKLOGIT (sink_logits: n_heads floats in device memory): heads_sink_logits_scan_kernel likewise ("scan_heads_sink_logits").
template <class E, bool WIN, bool SINK, bool GQA, bool ALIBI = false, bool SOFTCAP = false, bool SINKLOGIT = false>
static int launch_heads_scan_t(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                               int D, int H, int Hkv, int lg, int window, int n_sink, void* ws, size_t ws_bytes,
                               hipStream_t st, const float* slopes = nullptr, float cap = 0.f,
                               const float* sink_logits = nullptr) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const int span = SINK ? sink_span(S, window, n_sink) : WIN ? window_span(S, window) : S;
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, span, D, D / H * Hkv, H, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    // page pointers of the item | the waves' parked rows and statistics, later the row's (item, head) statistics
    const size_t smem = scan_lds_bytes(p.ct, heads_reduction_bytes(nj, E::EPL), heads_merge_stat_bytes(p.nchunk, H));
    if (!scan_lds_fits(smem)) return MLI_ERR_BAD_ARG;   // (kMaxMergeStats keeps every accepted shape far inside)
    count_launch(SINKLOGIT ? kLfScanHeadsSinkLogits
                 : SOFTCAP ? kLfScanHeadsSoftcap : ALIBI ? kLfScanHeadsAlibi : kLfScanHeadsWindow);
    dispatch_scan_variant<E>(ScanVariant{nj, false, 1}, p.nt, [&](auto NJ, auto, auto, auto NT) {
        if constexpr (SINKLOGIT)
            hipLaunchKernelGGL((heads_sink_logits_scan_kernel<E, NJ(), NT(), WIN, SINK, GQA>), dim3(B, p.grid_y),
                               dim3(kFuThreads), smem, st, q, page_table, lengths, out, w.ml, w.partial, S, D, lg, H, p.ct,
                               p.nchunk, p.direct, w.arrivals, window, n_sink, H / Hkv, sink_logits);
        else if constexpr (SOFTCAP)
            hipLaunchKernelGGL((heads_softcap_scan_kernel<E, NJ(), NT(), WIN, SINK, GQA>), dim3(B, p.grid_y), dim3(kFuThreads),
                               smem, st, q, page_table, lengths, out, w.ml, w.partial, S, D, lg, H, p.ct, p.nchunk, p.direct,
                               w.arrivals, window, n_sink, H / Hkv, cap);
        else if constexpr (ALIBI)
            hipLaunchKernelGGL((heads_alibi_scan_kernel<E, NJ(), NT(), WIN, SINK, GQA>), dim3(B, p.grid_y), dim3(kFuThreads),
                               smem, st, q, page_table, lengths, out, w.ml, w.partial, S, D, lg, H, p.ct, p.nchunk, p.direct,
                               w.arrivals, window, n_sink, H / Hkv, slopes);
        else
            hipLaunchKernelGGL((heads_decode_scan_kernel<E, NJ(), NT(), WIN, SINK, GQA>), dim3(B, p.grid_y), dim3(kFuThreads),
                               smem, st, q, page_table, lengths, out, w.ml, w.partial, S, D, lg, H, p.ct, p.nchunk, p.direct,
                               w.arrivals, window, n_sink, H / Hkv);
    });
    return launch_status();
}

// launch_lean_scan's multi-head scans: H > 1, lg = heads_lanes_log2 >= 0, Hkv a divisor of H (Hkv < H: GQA), the workspace
// body; kind = lean_scan_kind(S, window, n_sink), and the kernel is given no window or no sinks where the kind has none
template <class E>
int launch_heads_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D, int H,
                      int Hkv, int lg, ScanKind kind, int window, int n_sink, void* ws, size_t ws_bytes, hipStream_t st) {
    const auto go = [&](auto gqa) {
        constexpr bool GQA = decltype(gqa)::value;
        if (kind == kScanSinks)
            return launch_heads_scan_t<E, true, true, GQA>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, n_sink, ws, ws_bytes, st);
        if (kind == kScanWindow)
            return launch_heads_scan_t<E, true, false, GQA>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, 0, ws, ws_bytes, st);
        return launch_heads_scan_t<E, false, false, GQA>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, 0, 0, ws, ws_bytes, st);
    };
    return Hkv != H ? go(std::true_type{}) : go(std::false_type{});
}

}  // namespace mli
