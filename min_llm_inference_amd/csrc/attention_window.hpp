// EXTENSION: sliding-window attention, with or without attention sinks, for the single-head paged decode scan (lean form,
// chunked grid, in-kernel merge).  The multi-head forms are attention_heads.hpp's.
//   window = W, 1 <= W < n_sequence: row b attends slots [lo, L) with L = min(lengths[b], n_sequence), lo = max(0, L - W).
// The workgroup body is the single-head scan's own (scan_item_body.hpp) with its compile-time window switch on; only this
// header instantiates it that way.  What the switch changes:
//   - the row's first live page is p0 = lo / 16; its items are cut from token 16 * p0, so a row has at most
//     ceil(W / 16) + 1 live pages and the grid, the item size and the workspace traffic follow that span, not n_sequence;
//   - page pointers are staged from page_table[b][p0 + ...]: an entry below p0 is never read;
//   - in the first live page slots t < lo - 16 * p0 are masked exactly as the slots beyond the row are.
// SINK = true: n_sink = K >= 1 with K + W < n_sequence, the row attends its first K tokens as well -- slots s < L with
// s < K or s >= lo.  What that switch changes:
//   - the row is seen as two page runs: its ps = ceil(K / 16) sink pages, then the pages from the window's first one
//     (p0 = lo / 16) on; skip = max(0, p0 - ps) pages between them are dropped.  Items are cut over that virtual row of
//     L - 16 * skip <= 16 * (ceil(K / 16) + ceil(W / 16) + 1) tokens -- an item may straddle the joint --, and the grid, the
//     item size and the workspace traffic follow that span;
//   - page pointers are staged through the mapping (virtual page v -> v < ps ? v : v + skip): an entry inside the dropped
//     run is never read;
//   - slot t of physical page P is live iff t < nt and (16 P + t < K or 16 P + t >= lo): the hole lies inside one page
//     (p0 == ps - 1), straddles a page edge (p0 == ps) or is the dropped run; every virtual page keeps a live slot.
// The merge, the arrival counters and the workspace layout are the un-windowed ones.  W >= n_sequence and K + W >=
// n_sequence never come here: launch_lean_scan (compose.hip) takes them to the un-windowed scan.  fp32, bf16 and fp8 pages,
// each compiled in a file of its own (attention_window.hip, attention_window_bf16.hip, attention_window_fp8.hip: 16 kernels
// each) so that none is the longest step of a build.
//
//   grid = (B, items of the span + 1) rows fast, 256 threads; one launch, no combine kernel
#pragma once

#include "scan_item_body.hpp"
#include "scan_launch.hpp"
#include "scan_row_order.hpp"

namespace mli {

// n_sink: 0 without SINK
template <class E, int NJ, bool NT, int TBR, bool DS, int RPI, bool SINK>
__global__ __launch_bounds__(kFuThreads, 2) void window_decode_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int ct, int ml_per_row, int nchunk_max, int direct,
    unsigned* arrivals, int window, int n_sink) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // rows rotated by the item index: the items of one row spread over the XCDs (fused_decode_scan_kernel)
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<true, SINK>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window, n_sink);
    fused_scan_item<E, NJ, NT, TBR, DS, /*SCORES=*/false, RPI, /*WIN=*/true, SINK>(
        q, page_table, lengths, nullptr, out, ml, partial, S, D, ct, ml_per_row, nchunk_max, direct, arrivals, b, c, c == 0,
        (int)gridDim.x, smem_raw, window, n_sink);
}

// The un-windowed launcher's plan (scan_plan.hpp) at the span window and sinks leave; the workspace layout stays n_sequence's.
template <class E, bool SINK>
static int launch_window_decode_t(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                                  int D, int window, int n_sink, void* ws, size_t ws_bytes, hipStream_t st) {
    const ScanVariant v = plain_scan_variant(D, E::EPL);
    const int span = SINK ? sink_span(S, window, n_sink) : window_span(S, window);
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, span, D, 1, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    const size_t smem = scan_lds_bytes(p.ct, plain_reduction_bytes(v, E::EPL), window_merge_stat_bytes(p.nchunk));
    if (!scan_lds_fits(smem)) return MLI_ERR_BAD_ARG;   // a span of more items than the statistics' LDS holds: nothing launched
    count_launch(kLfScanHeadsWindow);
    dispatch_scan_variant<E>(v, p.nt, [&](auto NJ, auto DS, auto RPI, auto NT) {
        hipLaunchKernelGGL((window_decode_scan_kernel<E, NJ(), NT(), (NJ() == 1 ? 8 : 4) / RPI(), DS(), RPI(), SINK>),
                           dim3(B, p.grid_y), dim3(kFuThreads), smem, st, q, page_table, lengths, out, w.ml, w.partial, S, D,
                           p.ct, ceil_div_i(S, 64), p.nchunk, p.direct, w.arrivals, window, n_sink);
    });
    return launch_status();
}

// launch_lean_scan's single-head scans under a window: a shape window_plain_shape_ok accepts, 1 <= window < S, the workspace
// body; kind = lean_scan_kind(S, window, n_sink), kScanWindow or kScanSinks; without sinks the kernel is given none
template <class E>
int launch_window_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                         ScanKind kind, int window, int n_sink, void* ws, size_t ws_bytes, hipStream_t st) {
    return kind == kScanSinks
               ? launch_window_decode_t<E, true>(q, page_table, lengths, out, B, S, D, window, n_sink, ws, ws_bytes, st)
               : launch_window_decode_t<E, false>(q, page_table, lengths, out, B, S, D, window, 0, ws, ws_bytes, st);
}

}  // namespace mli
