// EXTENSION: attention sinks for the sliding-window paged decode scan (lean form, chunked grid, in-kernel merge).
//   n_sink = K >= 1, window = W >= 1, K + W < n_sequence: row b attends slots s < L with s < K or s >= lo,
//   L = min(lengths[b], n_sequence), lo = max(0, L - W) -- its first K tokens and its newest W.
// The workgroup bodies are the single-head and the multi-head scan's own (scan_item_body.hpp, heads_item_body.hpp) with
// their compile-time window AND sink switches on; only this file instantiates them that way.  What the sink switch changes:
//   - the row is seen as two page runs: its ps = ceil(K / 16) sink pages, then the pages from the window's first one
//     (p0 = lo / 16) on; skip = max(0, p0 - ps) pages between them are dropped.  Items are cut over that virtual row of
//     L - 16 * skip <= 16 * (ceil(K / 16) + ceil(W / 16) + 1) tokens -- an item may straddle the joint --, and the grid, the
//     item size and the workspace traffic follow that span;
//   - page pointers are staged through the mapping (virtual page v -> v < ps ? v : v + skip): an entry inside the dropped
//     run is never read;
//   - slot t of physical page P is live iff t < nt and (16 P + t < K or 16 P + t >= lo): the hole lies inside one page
//     (p0 == ps - 1), straddles a page edge (p0 == ps) or is the dropped run; every virtual page keeps a live slot.
// The merge, the arrival counters and the workspace layout are the un-windowed ones.  K == 0, K + W >= n_sequence and
// W >= n_sequence never come here: the entry points hand them to the existing ones unchanged.
//
//   grid = (B, items of the span + 1) rows fast, 256 threads; one launch, no combine kernel
#include "heads_item_body.hpp"
#include "scan_launch.hpp"
#include "scan_row_order.hpp"

namespace mli {

template <class E, int NJ, bool NT, int TBR, bool DS, int RPI>
__global__ __launch_bounds__(kFuThreads, 2) void sink_decode_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int ct, int ml_per_row, int nchunk_max, int direct,
    unsigned* arrivals, int window, int n_sink) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // rows rotated by the item index: the items of one row spread over the XCDs (fused_decode_scan_kernel)
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<true, true>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window, n_sink);
    fused_scan_item<E, NJ, NT, TBR, DS, false, RPI, true, true>(q, page_table, lengths, nullptr, out, ml, partial, S, D, ct,
                                                                ml_per_row, nchunk_max, direct, arrivals, b, c, c == 0,
                                                                (int)gridDim.x, smem_raw, window, n_sink);
}

template <class E, int NJ, bool NT>
__global__ __launch_bounds__(kFuThreads, 2) void sink_heads_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window, int n_sink) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<true, true>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window, n_sink);
    constexpr int PD = (NJ == 2 && E::EPL == 8) ? 2 : 3;   // heads_decode_scan_kernel
    heads_scan_item<E, NJ, NT, NJ == 1 ? 8 : 4, PD, true, true>(q, page_table, lengths, out, ml, partial, S, D, lg, H, ct,
                                                                nchunk_max, direct, arrivals, b, c, c == 0, smem_raw, window,
                                                                n_sink);
}

// The un-windowed launchers' plan (scan_plan.hpp) at the span sinks and window leave; the workspace layout stays n_sequence's.
template <class E>
static int launch_sink_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                              int D, int window, int n_sink, void* ws, size_t ws_bytes, hipStream_t st) {
    const ScanVariant v = plain_scan_variant(D, E::EPL);
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, sink_span(S, window, n_sink), D, 1, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    const size_t smem = scan_lds_bytes(p.ct, plain_reduction_bytes(v, E::EPL), window_merge_stat_bytes(p.nchunk));
    dispatch_scan_variant<E>(v, p.nt, [&](auto NJ, auto DS, auto RPI, auto NT) {
        hipLaunchKernelGGL((sink_decode_scan_kernel<E, NJ(), NT(), (NJ() == 1 ? 8 : 4) / RPI(), DS(), RPI()>), dim3(B, p.grid_y),
                           dim3(kFuThreads), smem, st, q, page_table, lengths, out, w.ml, w.partial, S, D, p.ct,
                           ceil_div_i(S, 64), p.nchunk, p.direct, w.arrivals, window, n_sink);
    });
    return launch_status();
}

template <class E>
static int launch_sink_heads(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                             int D, int H, int lg, int window, int n_sink, void* ws, size_t ws_bytes, hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, sink_span(S, window, n_sink), D, H, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    const size_t smem = scan_lds_bytes(p.ct, heads_reduction_bytes(nj, E::EPL), heads_merge_stat_bytes(p.nchunk, H));
    dispatch_scan_variant<E>(ScanVariant{nj, false, 1}, p.nt, [&](auto NJ, auto, auto, auto NT) {
        hipLaunchKernelGGL((sink_heads_scan_kernel<E, NJ(), NT()>), dim3(B, p.grid_y), dim3(kFuThreads), smem, st, q,
                           page_table, lengths, out, w.ml, w.partial, S, D, lg, H, p.ct, p.nchunk, p.direct, w.arrivals, window,
                           n_sink);
    });
    return launch_status();
}

// 1 <= n_sink, n_sink + window < n_sequence, shape already accepted by window_shape_supported
int launch_sink_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                     int H, int window, int n_sink, int elem, void* ws, size_t ws_bytes, hipStream_t st) {
    if (H > 1) {
        const int lg = heads_lanes_log2(B, S, D, H, elem);
        return elem == MLI_ELEM_BF16
                   ? launch_sink_heads<ElemBF16>(q, page_table, lengths, out, B, S, D, H, lg, window, n_sink, ws, ws_bytes, st)
                   : launch_sink_heads<ElemF32>(q, page_table, lengths, out, B, S, D, H, lg, window, n_sink, ws, ws_bytes, st);
    }
    if (elem == MLI_ELEM_FP8)
        return launch_sink_decode<ElemFP8>(q, page_table, lengths, out, B, S, D, window, n_sink, ws, ws_bytes, st);
    if (elem == MLI_ELEM_BF16)
        return launch_sink_decode<ElemBF16>(q, page_table, lengths, out, B, S, D, window, n_sink, ws, ws_bytes, st);
    return launch_sink_decode<ElemF32>(q, page_table, lengths, out, B, S, D, window, n_sink, ws, ws_bytes, st);
}

}  // namespace mli

extern "C" {

// hand-offs first: no sinks is the windowed call; no gap any row could have is the un-windowed one
int mli_decode_scan_paged_sinks(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int window,
                                int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_sink < 0 || window < 1 || n_heads < 1) return MLI_ERR_BAD_ARG;
    if (n_sink == 0)
        return mli_decode_scan_paged_window(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim,
                                            n_heads, window, elem, workspace, workspace_bytes, stream);
    if (mli::lean_scan_kind(n_sequence, window, n_sink) == mli::kScanPlain) {
        if (n_heads == 1)
            return mli_decode_scan_paged(q_output, page_table, lengths, nullptr, attention_result, n_batch, n_sequence,
                                         emb_dim, elem, 7, workspace, workspace_bytes, stream);
        return mli_decode_scan_paged_heads(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim,
                                           n_heads, elem, workspace, workspace_bytes, stream);
    }
    if (!mli::window_shape_supported(n_batch, n_sequence, emb_dim, n_heads, elem)) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                 n_heads, window, n_sink, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

// fill and projection depend neither on the window nor on the sinks
int mli_paged_attention_lean_sinks(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                   const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                   int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int window,
                                   int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (n_sink < 0 || window < 1 || n_heads < 1) return MLI_ERR_BAD_ARG;
    if (n_sink == 0)
        return mli_paged_attention_lean_window(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                               n_batch, n_sequence, emb_dim, n_new_items, n_heads, window, elem, workspace,
                                               workspace_bytes, stream);
    if (mli::lean_scan_kind(n_sequence, window, n_sink) == mli::kScanPlain) {
        if (n_heads == 1)
            return mli_paged_attention_lean(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                            n_batch, n_sequence, emb_dim, n_new_items, elem, workspace, workspace_bytes, stream);
        return mli_paged_attention_lean_heads(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                              n_batch, n_sequence, emb_dim, n_new_items, n_heads, elem, workspace,
                                              workspace_bytes, stream);
    }
    if (!mli::window_shape_supported(n_batch, n_sequence, emb_dim, n_heads, elem)) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_attention(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                      n_batch, n_sequence, emb_dim, n_new_items, n_heads, n_heads, window, n_sink, workspace,
                                      workspace_bytes, mli::as_stream(stream));
}

}  // extern "C"
