// EXTENSION: sliding-window attention for the paged decode scan (lean form, chunked grid, in-kernel merge).
//   window = W >= 1: row b attends slots [lo, L) with L = min(lengths[b], n_sequence), lo = max(0, L - W).
// The workgroup bodies are the single-head and the multi-head scan's own (scan_item_body.hpp, heads_item_body.hpp) with
// their compile-time window switch on; only this file instantiates them that way.  What the switch changes:
//   - the row's first live page is p0 = lo / 16; its items are cut from token 16 * p0, so a row has at most
//     ceil(W / 16) + 1 live pages and the grid, the item size and the workspace traffic follow that span, not n_sequence;
//   - page pointers are staged from page_table[b][p0 + ...]: an entry below p0 is never read;
//   - in the first live page slots t < lo - 16 * p0 are masked exactly as the slots beyond the row are.
// The merge, the arrival counters and the workspace layout are the un-windowed ones.  W >= n_sequence never comes here:
// the entry points hand it to the existing ones unchanged.
//
//   grid = (B, items of the span + 1) rows fast, 256 threads; one launch, no combine kernel
#include "heads_item_body.hpp"
#include "scan_launch.hpp"
#include "scan_row_order.hpp"

namespace mli {

template <class E, int NJ, bool NT, int TBR, bool DS, int RPI>
__global__ __launch_bounds__(kFuThreads, 2) void window_decode_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int ct, int ml_per_row, int nchunk_max, int direct,
    unsigned* arrivals, int window) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // rows rotated by the item index: the items of one row spread over the XCDs (fused_decode_scan_kernel)
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<true>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window);
    fused_scan_item<E, NJ, NT, TBR, DS, false, RPI, true>(q, page_table, lengths, nullptr, out, ml, partial, S, D, ct,
                                                          ml_per_row, nchunk_max, direct, arrivals, b, c, c == 0,
                                                          (int)gridDim.x, smem_raw, window);
}

template <class E, int NJ, bool NT>
__global__ __launch_bounds__(kFuThreads, 2) void window_heads_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<true>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window);
    constexpr int PD = (NJ == 2 && E::EPL == 8) ? 2 : 3;   // heads_decode_scan_kernel
    heads_scan_item<E, NJ, NT, NJ == 1 ? 8 : 4, PD, true>(q, page_table, lengths, out, ml, partial, S, D, lg, H, ct,
                                                          nchunk_max, direct, arrivals, b, c, c == 0, smem_raw, window);
}

// The un-windowed launchers' plan (scan_plan.hpp) at the span the window leaves; the workspace layout stays n_sequence's.
template <class E>
static int launch_window_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                                int D, int window, void* ws, size_t ws_bytes, hipStream_t st) {
    const ScanVariant v = plain_scan_variant(D, E::EPL);
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, window_span(S, window), D, 1, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    const size_t smem = scan_lds_bytes(p.ct, plain_reduction_bytes(v, E::EPL), window_merge_stat_bytes(p.nchunk));
    dispatch_scan_variant<E>(v, p.nt, [&](auto NJ, auto DS, auto RPI, auto NT) {
        hipLaunchKernelGGL((window_decode_scan_kernel<E, NJ(), NT(), (NJ() == 1 ? 8 : 4) / RPI(), DS(), RPI()>), dim3(B, p.grid_y),
                           dim3(kFuThreads), smem, st, q, page_table, lengths, out, w.ml, w.partial, S, D, p.ct,
                           ceil_div_i(S, 64), p.nchunk, p.direct, w.arrivals, window);
    });
    return launch_status();
}

template <class E>
static int launch_window_heads(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                               int D, int H, int lg, int window, void* ws, size_t ws_bytes, hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, window_span(S, window), D, H, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    const size_t smem = scan_lds_bytes(p.ct, heads_reduction_bytes(nj, E::EPL), heads_merge_stat_bytes(p.nchunk, H));
    dispatch_scan_variant<E>(ScanVariant{nj, false, 1}, p.nt, [&](auto NJ, auto, auto, auto NT) {
        hipLaunchKernelGGL((window_heads_scan_kernel<E, NJ(), NT()>), dim3(B, p.grid_y), dim3(kFuThreads), smem, st, q,
                           page_table, lengths, out, w.ml, w.partial, S, D, lg, H, p.ct, p.nchunk, p.direct, w.arrivals, window);
    });
    return launch_status();
}

// window < n_sequence, shape already accepted by window_shape_supported
int launch_window_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                       int H, int window, int elem, void* ws, size_t ws_bytes, hipStream_t st) {
    if (H > 1) {
        const int lg = heads_lanes_log2(B, S, D, H, elem);
        return elem == MLI_ELEM_BF16
                   ? launch_window_heads<ElemBF16>(q, page_table, lengths, out, B, S, D, H, lg, window, ws, ws_bytes, st)
                   : launch_window_heads<ElemF32>(q, page_table, lengths, out, B, S, D, H, lg, window, ws, ws_bytes, st);
    }
    if (elem == MLI_ELEM_FP8) return launch_window_decode<ElemFP8>(q, page_table, lengths, out, B, S, D, window, ws, ws_bytes, st);
    if (elem == MLI_ELEM_BF16) return launch_window_decode<ElemBF16>(q, page_table, lengths, out, B, S, D, window, ws, ws_bytes, st);
    return launch_window_decode<ElemF32>(q, page_table, lengths, out, B, S, D, window, ws, ws_bytes, st);
}

}  // namespace mli

extern "C" {

// window >= n_sequence is no window: the un-windowed entry points, with their own refusals
int mli_decode_scan_paged_window(const float* q_output, const void* const* page_table, const int* lengths,
                                 float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int window,
                                 int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (window < 1 || n_heads < 1) return MLI_ERR_BAD_ARG;
    if (window >= n_sequence) {
        if (n_heads == 1)
            return mli_decode_scan_paged(q_output, page_table, lengths, nullptr, attention_result, n_batch, n_sequence,
                                         emb_dim, elem, 7, workspace, workspace_bytes, stream);
        return mli_decode_scan_paged_heads(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim,
                                           n_heads, elem, workspace, workspace_bytes, stream);
    }
    if (!mli::window_shape_supported(n_batch, n_sequence, emb_dim, n_heads, elem)) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                 n_heads, window, 0, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

// fill and projection do not depend on the window
int mli_paged_attention_lean_window(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                    const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                    int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int window,
                                    int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (window < 1 || n_heads < 1) return MLI_ERR_BAD_ARG;
    if (window >= n_sequence) {
        if (n_heads == 1)
            return mli_paged_attention_lean(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                            n_batch, n_sequence, emb_dim, n_new_items, elem, workspace, workspace_bytes, stream);
        return mli_paged_attention_lean_heads(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                              n_batch, n_sequence, emb_dim, n_new_items, n_heads, elem, workspace,
                                              workspace_bytes, stream);
    }
    if (!mli::window_shape_supported(n_batch, n_sequence, emb_dim, n_heads, elem)) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_attention(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                      n_batch, n_sequence, emb_dim, n_new_items, n_heads, n_heads, window, 0, workspace,
                                      workspace_bytes,
                                      mli::as_stream(stream));
}

}  // extern "C"
