// EXTENSION: ALiBi, a linear position bias per query head, for the multi-head paged decode scan (attention_heads.hpp) in every
// one of its forms -- plain, WIN, WIN + SINK, each with or without GQA.
//   slopes: n_heads fp32 values in device memory, one per QUERY head (under GQA the g heads of a group read the same K/V and
//   carry different slopes), finite, of any sign.  For row b with L = min(lengths[b], n_sequence), query head h and an
//   attended slot s:   x[h][s] = (q_h . K_{h/g}[s]) / sqrtf(head_dim) + slopes[h] * (s - (L - 1))
//   s is the token's absolute slot in the row: not the position inside the page, the item, or the virtual row of sink pages
//   and window pages -- the gap under sinks counts towards the distance.  The bias is taken relative to the newest token: 0 at
//   s = L - 1 and, with the usual positive slopes, <= 0 everywhere, which keeps fp32 scores small where the probability
//   mass is.  (slope * s differs from it by a constant per row and head, which softmax does not see, but costs accuracy.)
// The attended set, the softmax and p . V are those of the scan without the bias; slopes all 0.0f give its bits.  What the
// switch adds to the workgroup body (heads_item_body.hpp: ALIBI) is one slope per lane load, one int -> float conversion per
// page and one fmaf per score between div_by and the page maximum.  Loads, prefetch, the all-reduce inside lane groups, masks,
// arrival counters, the per-head merge and the workspace layout are untouched: the bias is absolute in the row, so the
// (max, sum) of a row's items already live in one frame.  Plan, carve, LDS and dispatch are launch_heads_scan_t's; the
// launches are counted as "scan_heads_alibi".  fp32 and bf16 pages, each compiled in a file of its own (attention_alibi.hip,
// attention_alibi_bf16.hip: 24 kernels each).  One head, fp8 pages and the prompt scan have no bias.
#pragma once

#include "attention_heads.hpp"

namespace mli {

// launch_heads_scan with slopes: H > 1, lg = heads_lanes_log2 >= 0, Hkv a divisor of H, slopes != nullptr, the workspace body
template <class E>
int launch_heads_alibi_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                            int H, int Hkv, int lg, ScanKind kind, int window, int n_sink, const float* slopes, void* ws,
                            size_t ws_bytes, hipStream_t st) {
    const auto go = [&](auto gqa) {
        constexpr bool GQA = decltype(gqa)::value;
        if (kind == kScanSinks)
            return launch_heads_scan_t<E, true, true, GQA, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, n_sink, ws, ws_bytes, st, slopes);
        if (kind == kScanWindow)
            return launch_heads_scan_t<E, true, false, GQA, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, 0, ws, ws_bytes, st, slopes);
        return launch_heads_scan_t<E, false, false, GQA, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, 0, 0, ws, ws_bytes, st, slopes);
    };
    return Hkv != H ? go(std::true_type{}) : go(std::false_type{});
}

}  // namespace mli
