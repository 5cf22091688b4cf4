// EXTENSION: grouped-query attention for the multi-head paged decode scan (lean form, chunked grid, in-kernel merge).
//   n_heads = H query heads, n_kv_heads = Hkv K/V heads, 1 <= Hkv <= H, H % Hkv == 0, g = H / Hkv (any integer),
//   hd = emb_dim / H, Dkv = Hkv * hd.  Query head h owns columns [h * hd, (h + 1) * hd) of q_output and attention_result and
//   attends K/V head h / g, which owns columns [(h / g) * hd, (h / g + 1) * hd) of the K and the V segment of every page
//   slot; columns >= Dkv of those segments are never read.  One softmax per query head over q_h . K_{h/g} / sqrtf(hd).
// That is multi-head attention with H heads on pages whose K / V column block h is a copy of block h / g, and the workgroup
// body is the multi-head scan's own (heads_item_body.hpp) with its compile-time GQA switch on; only this file instantiates
// it that way.  What the switch changes is the 16-byte unit a lane loads (gqa_kv_unit, scan_plan.hpp): the lanes of the g
// query heads of a group issue the same addresses inside one load instruction, so the bytes fetched from memory fall by g
// while the load instructions do not.  Grid, item size, workspace, LDS, merge and arrival counters are those of H heads;
// the cache policy of the K / V loads is judged by the Dkv columns actually read.  Plain, windowed and with sinks
// (lean_scan_kind), fp32 and bf16 pages.  Hkv == H never comes here: the entry points hand it to the existing ones unchanged.
//
//   grid = (B, items of the span + 1) rows fast, 256 threads; one launch, no combine kernel
#include "heads_item_body.hpp"
#include "scan_launch.hpp"
#include "scan_row_order.hpp"

namespace mli {

template <class E, int NJ, bool NT, bool WIN, bool SINK>
__global__ __launch_bounds__(kFuThreads, 2) void gqa_heads_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window, int n_sink, int gq) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // rows rotated by the item index: the items of one row spread over the XCDs (fused_decode_scan_kernel)
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row<WIN, SINK>(lengths, (int)gridDim.x, S, (int)blockIdx.x, window, n_sink);
    constexpr int PD = (NJ == 2 && E::EPL == 8) ? 2 : 3;   // heads_decode_scan_kernel
    heads_scan_item<E, NJ, NT, NJ == 1 ? 8 : 4, PD, WIN, SINK, true>(q, page_table, lengths, out, ml, partial, S, D, lg, H, ct,
                                                                     nchunk_max, direct, arrivals, b, c, c == 0, smem_raw,
                                                                     window, n_sink, gq);
}

// The multi-head launchers' plan (scan_plan.hpp) at the span the scan kind leaves, read width Dkv.
template <class E, bool WIN, bool SINK>
static int launch_gqa_heads(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                            int H, int Hkv, int lg, int window, int n_sink, void* ws, size_t ws_bytes, hipStream_t st) {
    const int nj = ceil_div_i(D / E::EPL, kWave);   // 1 or 2
    const int span = SINK ? sink_span(S, window, n_sink) : WIN ? window_span(S, window) : S;
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, span, D, D / H * Hkv, H, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    const size_t smem = scan_lds_bytes(p.ct, heads_reduction_bytes(nj, E::EPL), heads_merge_stat_bytes(p.nchunk, H));
    dispatch_scan_variant<E>(ScanVariant{nj, false, 1}, p.nt, [&](auto NJ, auto, auto, auto NT) {
        hipLaunchKernelGGL((gqa_heads_scan_kernel<E, NJ(), NT(), WIN, SINK>), dim3(B, p.grid_y), dim3(kFuThreads), smem, st, q,
                           page_table, lengths, out, w.ml, w.partial, S, D, lg, H, p.ct, p.nchunk, p.direct, w.arrivals, window,
                           n_sink, H / Hkv);
    });
    return launch_status();
}

// Hkv < H, shape already accepted by gqa_shape_supported; kind = lean_scan_kind(S, window, n_sink)
int launch_gqa_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D, int H,
                    int Hkv, int window, int n_sink, int elem, void* ws, size_t ws_bytes, hipStream_t st) {
    const int lg = heads_lanes_log2(B, S, D, H, elem);
    if (lg < 0 || !gqa_shape_supported(B, S, D, H, Hkv, elem)) return MLI_ERR_BAD_ARG;
    const ScanKind kind = lean_scan_kind(S, window, n_sink);
    const auto go = [&](auto e) {
        using E = decltype(e);
        if (kind == kScanSinks)
            return launch_gqa_heads<E, true, true>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, n_sink, ws, ws_bytes, st);
        if (kind == kScanWindow)
            return launch_gqa_heads<E, true, false>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, window, 0, ws, ws_bytes, st);
        return launch_gqa_heads<E, false, false>(q, page_table, lengths, out, B, S, D, H, Hkv, lg, 0, 0, ws, ws_bytes, st);
    };
    return elem == MLI_ELEM_BF16 ? go(ElemBF16{}) : go(ElemF32{});
}

// what the two entry points refuse alike; 1 = n_kv_heads == n_heads, the existing entry point's call
static int gqa_args(int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int n_sink, int elem) {
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return MLI_ERR_BAD_ARG;
    if (n_sink < 0 || n_heads < 1 || n_kv_heads < 1 || n_kv_heads > n_heads || n_heads % n_kv_heads != 0) return MLI_ERR_BAD_ARG;
    if (n_kv_heads == n_heads) return 1;
    return gqa_shape_supported(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, elem) ? 0 : MLI_ERR_BAD_ARG;
}

}  // namespace mli

extern "C" {

// n_kv_heads == n_heads first: the entry point with sinks (no window is a window of n_sequence there), same kernels, same bits
int mli_decode_scan_paged_gqa(const float* q_output, const void* const* page_table, const int* lengths,
                              float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads,
                              int window, int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = mli::gqa_args(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, n_sink, elem);
    if (rc < 0) return rc;
    if (rc == 1) {
        if (n_sequence < 1) return MLI_ERR_BAD_ARG;
        return mli_decode_scan_paged_sinks(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim,
                                           n_heads, window < 1 ? n_sequence : window, n_sink, elem, workspace, workspace_bytes,
                                           stream);
    }
    return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                 n_kv_heads, window, n_sink, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

// fill and projection do not depend on n_kv_heads: the pages stay emb_dim wide, the scan reads their first Dkv K / V columns
int mli_paged_attention_lean_gqa(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                 const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                 int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                 int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = mli::gqa_args(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, n_sink, elem);
    if (rc < 0) return rc;
    if (rc == 1) {
        if (n_sequence < 1) return MLI_ERR_BAD_ARG;
        return mli_paged_attention_lean_sinks(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                              n_batch, n_sequence, emb_dim, n_new_items, n_heads,
                                              window < 1 ? n_sequence : window, n_sink, elem, workspace, workspace_bytes, stream);
    }
    return mli::launch_lean_attention(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result, n_batch,
                                      n_sequence, emb_dim, n_new_items, n_heads, n_kv_heads, window, n_sink, workspace,
                                      workspace_bytes, mli::as_stream(stream));
}

}  // extern "C"
