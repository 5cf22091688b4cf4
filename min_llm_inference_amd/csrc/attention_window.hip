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
#include "scan_row_order.hpp"

namespace mli {

int fused_chunk_tokens(int B, int S);   // attention_fused.hip
int scan_row_order();
int tuned_chunk_tokens();               // attention_scan.hip
int nt_loads_for(int B, int S, int D, int esize);
size_t stats_region_bytes_for(int B, int S);
int heads_lanes_log2(int B, int S, int D, int H, int elem);   // attention_heads.hip
int heads_chunk_tokens(int B, int S, int H);
size_t heads_stats_bytes(int B, int S, int H);

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

// The tokens a windowed row can span: its window plus the part of the first live page below it, whole pages.
static int window_span(int S, int window) {
    const int64_t span = (int64_t)kPage * (ceil_div_i(window, kPage) + 1);
    return span < S ? (int)span : S;
}

// One head: what the lean chunked scan takes (launch_fused_decode), with the rows the arrival counters can count.
static bool window_plain_shape_ok(int B, int S, int D, int elem) {
    if (B <= 0 || B > kMaxArrivalRows || S <= 0 || S % kPage != 0 || D <= 0) return false;
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16 && elem != MLI_ELEM_FP8) return false;
    const int epl = elem == MLI_ELEM_FP8 ? 16 : elem == MLI_ELEM_BF16 ? 8 : 4;
    if (D % epl != 0) return false;
    const int nj = ceil_div_i(D / epl, kWave);
    return elem == MLI_ELEM_FP8 ? nj <= 2 : nj <= 8;
}

int window_shape_supported(int n_batch, int n_sequence, int emb_dim, int n_heads, int elem) {   // engine_api.cpp
    if (n_heads < 1) return 0;
    return n_heads == 1 ? window_plain_shape_ok(n_batch, n_sequence, emb_dim, elem)
                        : heads_lanes_log2(n_batch, n_sequence, emb_dim, n_heads, elem) >= 0;
}

template <class E>
static int launch_window_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                                int D, int window, void* ws, size_t ws_bytes, hipStream_t st) {
    constexpr bool kFp8 = std::is_same<E, ElemFP8>::value;
    const int Du = D / E::EPL;
    const int nj = ceil_div_i(Du, kWave);
    const int rpi = kFp8 ? (Du <= 16 ? 4 : Du <= 32 ? 2 : 1) : 1;
    const bool dsplit = nj > 2;
    const int nj_ds = ceil_div_i(Du, kWave * kFuWaves);
    // grid and item size: launch_fused_decode's choices at the span the window leaves
    const int span = window_span(S, window);
    const int ct = (span <= 128 && B >= 256 && tuned_chunk_tokens() == 0) ? 128 : fused_chunk_tokens(B, span);
    const int nchunk = ceil_div_i(span, ct);
    const bool ordered = scan_row_order() && nchunk == 1 && B > 512 && B <= kMaxOrderedRows && span / kPage <= kMaxOrderedPages;
    const int direct = nchunk == 1 ? (ordered ? 2 : 1) : 0;
    // the un-windowed workspace layout: statistics with the row stride of n_sequence, then the partial rows
    const size_t stats_bytes = stats_region_bytes_for(B, S);
    const int ml_per_row = ceil_div_i(S, 64);
    float2* ml = nullptr;
    float* partial = nullptr;
    unsigned* arrivals = nullptr;
    if (!direct) {
        if (ws == nullptr || ws_bytes < stats_bytes + (size_t)B * nchunk * D * sizeof(float)) return MLI_ERR_WORKSPACE;
        ml = reinterpret_cast<float2*>(ws);
        partial = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + stats_bytes);
        arrivals = ws_arrivals(ws);
    }
    const size_t red_bytes = (dsplit ? (size_t)2 * kFuWaves * 16 : (size_t)kFuWaves * nj * (kWave / rpi) * E::EPL) * sizeof(float);
    const size_t stat_bytes_row = (size_t)nchunk * 8;
    const size_t smem = (size_t)(ct / kPage) * 8 + (red_bytes > stat_bytes_row ? red_bytes : stat_bytes_row);
    const dim3 grid(B, direct ? 1 : nchunk + 1);
    const bool nt = nt_loads_for(B, span, D, E::kBytes);
#define MLI_WIN_LAUNCH(NJ, DS, RPI)                                                                                       \
    do {                                                                                                                 \
        if (nt)                                                                                                          \
            hipLaunchKernelGGL((window_decode_scan_kernel<E, NJ, true, (NJ == 1 ? 8 : 4) / RPI, DS, RPI>), grid,         \
                               dim3(kFuThreads), smem, st, q, page_table, lengths, out, ml, partial, S, D, ct, ml_per_row, \
                               nchunk, direct, arrivals, window);                                                         \
        else                                                                                                             \
            hipLaunchKernelGGL((window_decode_scan_kernel<E, NJ, false, (NJ == 1 ? 8 : 4) / RPI, DS, RPI>), grid,        \
                               dim3(kFuThreads), smem, st, q, page_table, lengths, out, ml, partial, S, D, ct, ml_per_row, \
                               nchunk, direct, arrivals, window);                                                         \
    } while (0)
    if constexpr (kFp8) {
        if (rpi == 4) MLI_WIN_LAUNCH(1, false, 4);
        else if (rpi == 2) MLI_WIN_LAUNCH(1, false, 2);
        else if (nj == 1) MLI_WIN_LAUNCH(1, false, 1);
        else MLI_WIN_LAUNCH(2, false, 1);
    } else if (dsplit) {
        if (nj_ds == 1) MLI_WIN_LAUNCH(1, true, 1);
        else MLI_WIN_LAUNCH(2, true, 1);
    } else if (nj == 1) {
        MLI_WIN_LAUNCH(1, false, 1);
    } else {
        MLI_WIN_LAUNCH(2, false, 1);
    }
#undef MLI_WIN_LAUNCH
    return launch_status();
}

template <class E>
static int launch_window_heads(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                               int D, int H, int lg, int window, void* ws, size_t ws_bytes, hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const int span = window_span(S, window);
    const int ct = heads_chunk_tokens(B, span, H);
    const int nchunk = ceil_div_i(span, ct);
    const bool ordered = scan_row_order() && nchunk == 1 && B > 512 && B <= kMaxOrderedRows && span / kPage <= kMaxOrderedPages;
    const int direct = nchunk == 1 ? (ordered ? 2 : 1) : 0;
    float2* ml = nullptr;
    float* partial = nullptr;
    unsigned* arrivals = nullptr;
    if (!direct) {
        const size_t stats_bytes = heads_stats_bytes(B, S, H);   // the un-windowed layout
        if (ws == nullptr || ws_bytes < stats_bytes + (size_t)B * nchunk * D * sizeof(float)) return MLI_ERR_WORKSPACE;
        ml = reinterpret_cast<float2*>(ws);
        partial = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + stats_bytes);
        arrivals = ws_arrivals(ws);
    }
    const size_t park_bytes = (size_t)kFuWaves * nj * kWave * (E::EPL * sizeof(float) + sizeof(float2));
    const size_t stat_bytes = (size_t)nchunk * H * sizeof(float2);
    const size_t smem = (size_t)(ct / kPage) * 8 + (park_bytes > stat_bytes ? park_bytes : stat_bytes);
    const dim3 grid(B, direct ? 1 : nchunk + 1);
    const bool nt = nt_loads_for(B, span, D, E::kBytes);
#define MLI_WIN_HEADS_LAUNCH(NJ, NT)                                                                                      \
    hipLaunchKernelGGL((window_heads_scan_kernel<E, NJ, NT>), grid, dim3(kFuThreads), smem, st, q, page_table, lengths, out, \
                       ml, partial, S, D, lg, H, ct, nchunk, direct, arrivals, window)
    if (nj == 1) {
        if (nt) MLI_WIN_HEADS_LAUNCH(1, true);
        else MLI_WIN_HEADS_LAUNCH(1, false);
    } else {
        if (nt) MLI_WIN_HEADS_LAUNCH(2, true);
        else MLI_WIN_HEADS_LAUNCH(2, false);
    }
#undef MLI_WIN_HEADS_LAUNCH
    return launch_status();
}

// window < n_sequence, shape already accepted by window_shape_supported
static int launch_window_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                              int D, int H, int window, int elem, void* workspace, size_t workspace_bytes, hipStream_t st) {
    const WsBody body = ws_body(workspace, workspace_bytes);
    if (H > 1) {
        const int lg = heads_lanes_log2(B, S, D, H, elem);
        return elem == MLI_ELEM_BF16
                   ? launch_window_heads<ElemBF16>(q, page_table, lengths, out, B, S, D, H, lg, window, body.ptr, body.bytes, st)
                   : launch_window_heads<ElemF32>(q, page_table, lengths, out, B, S, D, H, lg, window, body.ptr, body.bytes, st);
    }
    if (elem == MLI_ELEM_FP8)
        return launch_window_decode<ElemFP8>(q, page_table, lengths, out, B, S, D, window, body.ptr, body.bytes, st);
    if (elem == MLI_ELEM_BF16)
        return launch_window_decode<ElemBF16>(q, page_table, lengths, out, B, S, D, window, body.ptr, body.bytes, st);
    return launch_window_decode<ElemF32>(q, page_table, lengths, out, B, S, D, window, body.ptr, body.bytes, st);
}

}  // namespace mli

extern "C" {

int mli_decode_scan_paged_window(const float* q_output, const void* const* page_table, const int* lengths,
                                 float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int window,
                                 int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (window < 1 || n_heads < 1) return MLI_ERR_BAD_ARG;
    if (window >= n_sequence) {   // no window: today's code paths, unchanged
        if (n_heads == 1)
            return mli_decode_scan_paged(q_output, page_table, lengths, nullptr, attention_result, n_batch, n_sequence,
                                         emb_dim, elem, 7, workspace, workspace_bytes, stream);
        return mli_decode_scan_paged_heads(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim,
                                           n_heads, elem, workspace, workspace_bytes, stream);
    }
    if (!mli::window_shape_supported(n_batch, n_sequence, emb_dim, n_heads, elem)) return MLI_ERR_BAD_ARG;
    return mli::launch_window_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                   window, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

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
    hipStream_t st = mli::as_stream(stream);
    // fill and projection: the launches of mli_paged_attention_lean (pages and q_output do not depend on the window)
    const int rc = mli::launch_fill_and_latest(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, n_batch,
                                               n_sequence, emb_dim, n_new_items, st);
    if (rc) return rc;
    return mli::launch_window_scan(q_output, reinterpret_cast<const void* const*>(page_table), lengths, attention_result,
                                   n_batch, n_sequence, emb_dim, n_heads, window, elem, workspace, workspace_bytes, st);
}

}  // extern "C"
