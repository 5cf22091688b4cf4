// EXTENSION: multi-head attention for the paged decode scan (lean form, chunked grid, in-kernel merge).
//   n_heads = H, head_dim = hd = emb_dim / H; head h owns columns [h * hd, (h + 1) * hd) of q_output and of the K and V
//   segments of every page slot; one softmax per head over q_h . K_h / sqrtf(hd).
// The scan reads exactly the bytes the single-head scan reads, with the same grid, prefetch and hand-off; the workgroup
// body (heads_item_body.hpp) keeps its softmax state per head.  H == 1 never comes here: the entry points hand it to
// the single-head code path unchanged.
//
//   grid = (B, chunks + 1) rows fast, 256 threads, a wave owns whole pages; one launch, no combine kernel
#include "heads_item_body.hpp"
#include "scan_row_order.hpp"

namespace mli {

int fused_chunk_tokens(int B, int S);   // attention_fused.hip
int scan_row_order();
int tuned_chunk_tokens();               // attention_scan.hip
int nt_loads_for(int B, int S, int D, int esize);

template <class E, int NJ, bool NT>
__global__ __launch_bounds__(kFuThreads, 2) void heads_decode_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // rows rotated by the chunk index: the chunks of one row spread over the XCDs (fused_decode_scan_kernel)
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row(lengths, (int)gridDim.x, S, (int)blockIdx.x);
    // 8 token slots per batch for rows of one lane load, 4 for rows of two; three batches in flight, except bf16 rows of
    // two lane loads: their 16 + 16 floats of q and output and 32 probabilities leave room for two live batches beside the
    // one being consumed without spilling
    constexpr int PD = (NJ == 2 && E::EPL == 8) ? 2 : 3;
    heads_scan_item<E, NJ, NT, NJ == 1 ? 8 : 4, PD>(q, page_table, lengths, out, ml, partial, S, D, lg, H, ct, nchunk_max,
                                                    direct, arrivals, b, c, c == 0, smem_raw);
}

constexpr int kMaxItemTokens = 1024;
constexpr int kMaxMergeStats = 4096;   // float2 entries

// The supported combinations (everything else is MLI_ERR_BAD_ARG before anything is launched).  Returns log2 of the lanes
// per head, or -1.  (This and the two sizing rules below: also attention_window.hip.)
int heads_lanes_log2(int B, int S, int D, int H, int elem) {
    if (B <= 0 || B > kMaxArrivalRows || S <= 0 || S % kPage != 0 || D <= 0 || H < 1 || D % H != 0) return -1;
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return -1;
    const int hd = D / H;
    if (hd != 32 && hd != 64 && hd != 128 && hd != 256) return -1;
    const int epl = elem == MLI_ELEM_BF16 ? 8 : 4;
    if (D / epl > 2 * kWave) return -1;   // rows of at most two lane loads: whole pages per wave
    // the last arriver stages a row's (items x heads) statistics in LDS: even at the largest item size they must fit
    if ((int64_t)ceil_div_i(S, kMaxItemTokens) * H > kMaxMergeStats) return -1;
    int lg = 0;
    while ((epl << lg) < hd) ++lg;
    return lg;
}

int heads_shape_supported(int n_batch, int n_sequence, int emb_dim, int n_heads, int elem) {   // engine_api.cpp
    return heads_lanes_log2(n_batch, n_sequence, emb_dim, n_heads, elem) >= 0;
}

// Tokens per item: the single-head scan's choice, raised where a row's (items x heads) statistics would not fit the
// 32 KiB of LDS the last arriver stages them in (n_sequence 16384 with 32 heads and a small batch).  A size exists for
// every shape heads_lanes_log2 accepts.
int heads_chunk_tokens(int B, int S, int H) {
    int ct = (S <= 128 && B >= 256 && tuned_chunk_tokens() == 0) ? 128 : fused_chunk_tokens(B, S);
    while (ct < kMaxItemTokens && (int64_t)ceil_div_i(S, ct) * H > kMaxMergeStats) ct <<= 1;
    return ct;
}

// body = [(m, l) per row, item and head: B * ceil(S / 64) * H float2, 256-B aligned][partial rows: B * ceil(S / 64) * D]
size_t heads_stats_bytes(int B, int S, int H) {
    const size_t n = (size_t)B * ceil_div_i(S, 64) * H * sizeof(float2);
    return (n + 255) & ~(size_t)255;
}

template <class E>
static int launch_heads_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                               int D, int H, int lg, void* ws, size_t ws_bytes, hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const int ct = heads_chunk_tokens(B, S, H);
    const int nchunk = ceil_div_i(S, ct);
    const bool ordered = scan_row_order() && nchunk == 1 && B > 512 && B <= kMaxOrderedRows && S / kPage <= kMaxOrderedPages;
    const int direct = nchunk == 1 ? (ordered ? 2 : 1) : 0;
    float2* ml = nullptr;
    float* partial = nullptr;
    unsigned* arrivals = nullptr;
    if (!direct) {
        const size_t stats_bytes = heads_stats_bytes(B, S, H);
        if (ws == nullptr || ws_bytes < stats_bytes + (size_t)B * nchunk * D * sizeof(float)) return MLI_ERR_WORKSPACE;
        ml = reinterpret_cast<float2*>(ws);
        partial = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + stats_bytes);
        arrivals = ws_arrivals(ws);
    }
    // page pointers of the item | the waves' parked rows and statistics, later the row's (item, head) statistics
    const size_t park_bytes = (size_t)kFuWaves * nj * kWave * (E::EPL * sizeof(float) + sizeof(float2));
    const size_t stat_bytes = (size_t)nchunk * H * sizeof(float2);
    const size_t smem = (size_t)(ct / kPage) * 8 + (park_bytes > stat_bytes ? park_bytes : stat_bytes);
    const dim3 grid(B, direct ? 1 : nchunk + 1);
    const bool nt = nt_loads_for(B, S, D, E::kBytes);
#define MLI_HEADS_LAUNCH(NJ, NT)                                                                                          \
    hipLaunchKernelGGL((heads_decode_scan_kernel<E, NJ, NT>), grid, dim3(kFuThreads), smem, st, q, page_table, lengths, out, \
                       ml, partial, S, D, lg, H, ct, nchunk, direct, arrivals)
    if (nj == 1) {
        if (nt) MLI_HEADS_LAUNCH(1, true);
        else MLI_HEADS_LAUNCH(1, false);
    } else {
        if (nt) MLI_HEADS_LAUNCH(2, true);
        else MLI_HEADS_LAUNCH(2, false);
    }
#undef MLI_HEADS_LAUNCH
    return launch_status();
}

static int launch_heads_decode_elem(const float* q, const void* const* page_table, const int* lengths, float* out, int B,
                                    int S, int D, int H, int lg, int elem, void* workspace, size_t workspace_bytes,
                                    hipStream_t st) {
    const WsBody body = ws_body(workspace, workspace_bytes);
    return elem == MLI_ELEM_BF16
               ? launch_heads_decode<ElemBF16>(q, page_table, lengths, out, B, S, D, H, lg, body.ptr, body.bytes, st)
               : launch_heads_decode<ElemF32>(q, page_table, lengths, out, B, S, D, H, lg, body.ptr, body.bytes, st);
}

}  // namespace mli

extern "C" {

size_t mli_attention_heads_workspace_bytes(int n_batch, int n_sequence, int dim, int n_heads) {
    if (n_heads == 1) return mli_attention_workspace_bytes(n_batch, n_sequence, dim);
    // either page element type: the layout does not depend on it
    if (mli::heads_lanes_log2(n_batch, n_sequence, dim, n_heads, MLI_ELEM_F32) < 0 &&
        mli::heads_lanes_log2(n_batch, n_sequence, dim, n_heads, MLI_ELEM_BF16) < 0)
        return 0;
    const size_t nchunk = (size_t)mli::ceil_div_i(n_sequence, 64);
    const size_t heads = mli::kArrivalRegionBytes + mli::heads_stats_bytes(n_batch, n_sequence, n_heads) +
                         (nchunk <= 1 ? 0 : (size_t)n_batch * nchunk * (size_t)dim * sizeof(float));
    const size_t plain = mli_attention_workspace_bytes(n_batch, n_sequence, dim);
    return heads > plain ? heads : plain;
}

int mli_decode_scan_paged_heads(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int elem,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return MLI_ERR_BAD_ARG;
    if (n_heads == 1)   // today's code path, unchanged
        return mli_decode_scan_paged(q_output, page_table, lengths, nullptr, attention_result, n_batch, n_sequence, emb_dim,
                                     elem, 7, workspace, workspace_bytes, stream);
    const int lg = mli::heads_lanes_log2(n_batch, n_sequence, emb_dim, n_heads, elem);
    if (lg < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_heads_decode_elem(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim,
                                         n_heads, lg, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

int mli_paged_attention_lean_heads(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                   const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                   int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int elem,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return MLI_ERR_BAD_ARG;
    if (n_heads == 1)
        return mli_paged_attention_lean(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result, n_batch,
                                        n_sequence, emb_dim, n_new_items, elem, workspace, workspace_bytes, stream);
    const int lg = mli::heads_lanes_log2(n_batch, n_sequence, emb_dim, n_heads, elem);
    if (lg < 0) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    // fill and projection: the launches of mli_paged_attention_lean (pages and q_output do not depend on n_heads)
    const int rc = mli::launch_fill_and_latest(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, n_batch,
                                               n_sequence, emb_dim, n_new_items, st);
    if (rc) return rc;
    return mli::launch_heads_decode_elem(q_output, reinterpret_cast<const void* const*>(page_table), lengths,
                                         attention_result, n_batch, n_sequence, emb_dim, n_heads, lg, elem, workspace,
                                         workspace_bytes, st);
}

}  // extern "C"
