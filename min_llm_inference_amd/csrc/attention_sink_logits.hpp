// EXTENSION: learned attention-sink logits for the multi-head paged decode scan (attention_heads.hpp) in every one of its forms
// -- plain, WIN, WIN + SINK, each with or without GQA -- and for the causal multi-query prompt scan (attention_prompt.hpp).
//   sink_logits: n_heads fp32 values in DEVICE memory, each finite or -inf.  For row b with L = min(lengths[b], n_sequence) >= 1,
//   query head h, K/V head h / g, the attended set A of the form and the scaled scores x_s = q_h . K_{h/g}[s] / sqrtf(head_dim):
//       m     = max( max_{s in A} x_s , z_h )
//       out_h = sum_{s in A} exp(x_s - m) V_{h/g}[s]  /  ( sum_{s in A} exp(x_s - m) + exp(z_h - m) )
//   (the per-head sink of the gpt-oss attention block; z_h = 0 for every head is the "off-by-one" softmax).  z_h is one more
//   logit of head h's softmax WITHOUT a value row: its probability mass is dropped.  It is the QUERY head's logit (the heads of a
//   K/V group differ), it is not scaled by 1 / sqrt(head_dim), no window masks it, and it counts ONCE per (row, head) however
//   many items or waves the row is split into.  It is not the n_sink switch (SINK), which keeps the first tokens of a row
//   attended; the two are used together.
// Where it enters (heads_item_body.hpp: SINKLOGIT): only where a row's final (m, l) of a head is formed -- the wave merge of a
// row that one workgroup scans (direct 1 and 2), or the last arriver's merge over the row's items.  What an item publishes, the
// page loop, the prefetch, the plan, the workspace, the LDS size and the arrival counters are launch_heads_scan_t's, untouched:
// the switch costs one 4-byte load, one fmaxf, one expf and one add per (thread, merge).
// Anchors: z_h = -inf is no sink and gives the _gqa kernel's bits (fmaxf(m, -inf) = m, l + expf(-inf) = l + 0); so does any
// logit so far below the scores that expf(z - m) is 0 (-1e30); a logit far above them (+1e30) gives exactly 0.0f on every
// non-empty row, because the maximum takes the sink in before any expf of a difference.  +inf and NaN are outside the contract.
// L == 0 gives the zero row as before.  The launches are counted as "scan_heads_sink_logits".  fp32 and bf16 pages, each
// compiled in a file of its own (attention_sink_logits.hip, attention_sink_logits_bf16.hip: 24 kernels each).  Not combined
// with ALiBi or soft-capping: no model defines that.  One head and fp8 pages have no sink logit.
#pragma once

#include "attention_heads.hpp"

namespace mli {

// launch_heads_scan with sink logits: H > 1, lg = heads_lanes_log2 >= 0, Hkv a divisor of H, sink_logits non-null, the
// workspace body
template <class E>
int launch_heads_sink_logits_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                                  int D, int H, int Hkv, int lg, ScanKind kind, int window, int n_sink, const float* sink_logits,
                                  void* ws, size_t ws_bytes, hipStream_t st) {
    const auto go = [&](auto gqa) {
        constexpr bool GQA = decltype(gqa)::value;
        if (kind == kScanSinks)
            return launch_heads_scan_t<E, true, true, GQA, false, false, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, n_sink, ws, ws_bytes, st, nullptr, 0.f, sink_logits);
        if (kind == kScanWindow)
            return launch_heads_scan_t<E, true, false, GQA, false, false, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, 0, ws, ws_bytes, st, nullptr, 0.f, sink_logits);
        return launch_heads_scan_t<E, false, false, GQA, false, false, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, 0, 0, ws, ws_bytes, st, nullptr, 0.f, sink_logits);
    };
    return Hkv != H ? go(std::true_type{}) : go(std::false_type{});
}

}  // namespace mli
