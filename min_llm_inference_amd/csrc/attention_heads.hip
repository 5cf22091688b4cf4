// EXTENSION: multi-head attention for the paged decode scan (lean form, chunked grid, in-kernel merge).
//   n_heads = H, head_dim = hd = emb_dim / H; head h owns columns [h * hd, (h + 1) * hd) of q_output and of the K and V
//   segments of every page slot; one softmax per head over q_h . K_h / sqrtf(hd).
// The scan reads exactly the bytes the single-head scan reads, with the same grid, prefetch and hand-off; the workgroup
// body (heads_item_body.hpp) keeps its softmax state per head.  H == 1 never comes here: the entry points hand it to
// the single-head code path unchanged.
//
//   grid = (B, chunks + 1) rows fast, 256 threads, a wave owns whole pages; one launch, no combine kernel
#include "heads_item_body.hpp"
#include "scan_launch.hpp"
#include "scan_row_order.hpp"

namespace mli {

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

// Grid, item size, workspace and LDS: scan_plan.hpp (the supported shapes: heads_lanes_log2 there).
template <class E>
static int launch_heads_decode_t(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                                 int D, int H, int lg, void* ws, size_t ws_bytes, hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, S, D, H, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    // page pointers of the item | the waves' parked rows and statistics, later the row's (item, head) statistics
    const size_t smem = scan_lds_bytes(p.ct, heads_reduction_bytes(nj, E::EPL), heads_merge_stat_bytes(p.nchunk, H));
    dispatch_scan_variant<E>(ScanVariant{nj, false, 1}, p.nt, [&](auto NJ, auto, auto, auto NT) {
        hipLaunchKernelGGL((heads_decode_scan_kernel<E, NJ(), NT()>), dim3(B, p.grid_y), dim3(kFuThreads), smem, st, q,
                           page_table, lengths, out, w.ml, w.partial, S, D, lg, H, p.ct, p.nchunk, p.direct, w.arrivals);
    });
    return launch_status();
}

int launch_heads_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                        int H, int elem, void* ws, size_t ws_bytes, hipStream_t st) {
    const int lg = heads_lanes_log2(B, S, D, H, elem);
    if (lg < 0) return MLI_ERR_BAD_ARG;
    return elem == MLI_ELEM_BF16 ? launch_heads_decode_t<ElemBF16>(q, page_table, lengths, out, B, S, D, H, lg, ws, ws_bytes, st)
                                 : launch_heads_decode_t<ElemF32>(q, page_table, lengths, out, B, S, D, H, lg, ws, ws_bytes, st);
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
    const size_t heads = mli::kArrivalRegionBytes + mli::scan_stats_bytes(n_batch, n_sequence, n_heads) +
                         (nchunk <= 1 ? 0 : (size_t)n_batch * nchunk * (size_t)dim * sizeof(float));
    const size_t plain = mli_attention_workspace_bytes(n_batch, n_sequence, dim);
    return heads > plain ? heads : plain;
}

// n_heads == 1 is the single-head scan (mli_decode_scan_paged, phases 7), unchanged
int mli_decode_scan_paged_heads(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int elem,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return MLI_ERR_BAD_ARG;
    if (n_heads != 1 && mli::heads_lanes_log2(n_batch, n_sequence, emb_dim, n_heads, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                 n_heads, 0, 0, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

// n_heads == 1 is mli_paged_attention_lean; fill and projection do not depend on n_heads
int mli_paged_attention_lean_heads(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                   const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                   int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int elem,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return MLI_ERR_BAD_ARG;
    if (n_heads != 1 && mli::heads_lanes_log2(n_batch, n_sequence, emb_dim, n_heads, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_attention(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                      n_batch, n_sequence, emb_dim, n_new_items, n_heads, n_heads, 0, 0, workspace, workspace_bytes,
                                      mli::as_stream(stream));
}

}  // extern "C"
