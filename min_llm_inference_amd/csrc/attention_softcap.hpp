// EXTENSION: attention logit soft-capping for the multi-head paged decode scan (attention_heads.hpp) in every one of its
// forms -- plain, WIN, WIN + SINK, each with or without GQA -- and for the causal multi-query prompt scan (attention_prompt.hpp).
//   cap: one finite fp32 value > 0 per call, a host value passed as a kernel argument.  For row b with
//   L = min(lengths[b], n_sequence), query head h, g = n_heads / n_kv_heads and an attended slot s:
//       x[h][s] = cap * tanh( ((q_h . K_{h/g}[s]) / sqrtf(head_dim)) / cap )
//   (the logits_soft_cap / attn_logit_softcapping argument of other serving stacks; Gemma 2, Grok-1).
// The cap is applied to the SCALED score: after div_by and the all-reduce inside the lane group, before the liveness mask
// and the page maximum.  A masked slot stays excluded -- the mask is a select on slot_live, so tanh(-inf) = -1 never turns a
// dead slot into a finite score of -cap, and whatever a dead slot's bytes score is dropped.  The cap is a pure function of
// the score, so the (max, sum) of a row's items live in one frame: plan, carve, workspace, per-head merge and arrival counters
// are launch_heads_scan_t's, untouched.  There is no zero element: no cap gives back the uncapped bits.  L == 1, and a
// one-slot window without sinks, give V's row L - 1 bit for bit whatever the cap (one probability, exp(0) / 1).
// What the switch adds to the workgroup body (heads_item_body.hpp: SOFTCAP, softcap_score) is about twenty VALU instructions
// per score, two of them transcendental, and no register that lives across a page.  The launches are counted as
// "scan_heads_softcap".  fp32 and bf16 pages, each compiled in a file of its own (attention_softcap.hip,
// attention_softcap_bf16.hip: 24 kernels each).  Not combined with ALiBi: the order of bias and cap would be an invention.
// One head and fp8 pages have no cap.
#pragma once

#include "attention_heads.hpp"

namespace mli {

// launch_heads_scan with a cap: H > 1, lg = heads_lanes_log2 >= 0, Hkv a divisor of H, cap > 0 finite, the workspace body
template <class E>
int launch_heads_softcap_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                              int H, int Hkv, int lg, ScanKind kind, int window, int n_sink, float cap, void* ws, size_t ws_bytes,
                              hipStream_t st) {
    const auto go = [&](auto gqa) {
        constexpr bool GQA = decltype(gqa)::value;
        if (kind == kScanSinks)
            return launch_heads_scan_t<E, true, true, GQA, false, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, n_sink, ws, ws_bytes, st, nullptr, cap);
        if (kind == kScanWindow)
            return launch_heads_scan_t<E, true, false, GQA, false, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, 0, ws, ws_bytes, st, nullptr, cap);
        return launch_heads_scan_t<E, false, false, GQA, false, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, 0, 0, ws, ws_bytes, st, nullptr, cap);
    };
    return Hkv != H ? go(std::true_type{}) : go(std::false_type{});
}

}  // namespace mli
