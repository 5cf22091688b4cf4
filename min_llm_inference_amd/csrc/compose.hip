// Compositions: the reference's inference_self_attention / paged_attention[_with_cublas] call
// order, issued back to back on one stream.
//   src/kernels/self_attention_inference_optimized.cu:282-301
//   src/kernels/paged_attention.cu:358-377, src/kernels/paged_attention_cublas.cu:260-280
#include <cmath>

#include "scan_launch.hpp"

namespace mli {
int launch_latest_naive(const float*, const int*, const float*, const float*, const float*, float*, float*, float*,
                        int, int, int, int, hipStream_t);
int launch_fill_naive(const float*, const int*, const int*, const float*, const float*, float*, float*, int, int, int,
                      int, int, hipStream_t);
int launch_latest_paged(float* const*, const int*, const float*, const float*, const float*, float*, int, int, int,
                        hipStream_t);
int launch_fill_paged(float* const*, const int*, const int*, const float*, const float*, int, int, int, int,
                      hipStream_t);
int launch_qkt_paged(const float*, const float* const*, const int*, float*, int, int, int, hipStream_t);
int launch_qkt_naive(const float*, const float*, const int*, float*, int, int, int, hipStream_t);
int launch_softmax(float*, const int*, int, int, hipStream_t);
int launch_softmax_v_naive(const float*, const float*, const int*, float*, int, int, int, void*, size_t, hipStream_t);
int launch_softmax_v_paged(const float*, const float* const*, const int*, float*, int, int, int, void*, size_t,
                           hipStream_t);
int launch_scores_softmax_v_paged(const float*, const float* const*, const int*, float*, float*, int, int, int, void*,
                                  size_t, hipStream_t);
int launch_scores_softmax_v_naive(const float*, const float*, const float*, const int*, float*, float*, int, int, int,
                                  void*, size_t, hipStream_t);
int launch_scores_softmax_v_paged_bf16(const float*, const uint16_t* const*, const int*, float*, float*, int, int, int,
                                       void*, size_t, hipStream_t);
// single-pass fused scan (attention_fused.hip): 1 = ran, 0 = not applicable (caller falls back), else error + (rc > 0)
int launch_fused_decode_f32(const float*, const float* const*, const int*, float*, float*, int, int, int, void*, size_t,
                            hipStream_t);
int launch_fused_decode_bf16(const float*, const uint16_t* const*, const int*, float*, float*, int, int, int, void*,
                             size_t, hipStream_t);
int launch_latest_paged_bf16(uint16_t* const*, const int*, const uint16_t*, const uint16_t*, const uint16_t*, float*, int,
                             int, int, hipStream_t);
int launch_fill_paged_bf16(uint16_t* const*, const int*, const int*, const uint16_t*, const uint16_t*, int, int, int,
                           int, hipStream_t);
int launch_fill_paged_embed(const float*, const float*, const int*, float* const*, const int*, const int*, const float*,
                            const float*, int, int, int, int, hipStream_t);
int launch_fill_paged_bf16_embed(const float*, const float*, const int*, uint16_t* const*, const int*, const int*,
                                 const uint16_t*, const uint16_t*, int, int, int, int, hipStream_t);
bool prefill_fuses(int emb_dim);   // proj_gemm.hip: mli_tune "prefill_fused"
// the windowed prefill (mli_paged_prefill_window): the same launches over a row's live tokens (page_live.hpp)
int launch_fill_paged_window_embed(const float*, const float*, const int*, float* const*, const int*, const int*, const float*,
                                   const float*, int, int, int, int, int, int, hipStream_t);
int launch_fill_paged_bf16_window_embed(const float*, const float*, const int*, uint16_t* const*, const int*, const int*,
                                        const uint16_t*, const uint16_t*, int, int, int, int, int, int, hipStream_t);
int launch_fill_paged_bf16_window(uint16_t* const*, const int*, const int*, const uint16_t*, const uint16_t*, int, int, int,
                                  int, int, int, hipStream_t);
int launch_fill_paged_fp8_window_embed(const float*, const float*, const int*, uint8_t* const*, const int*, const int*,
                                       const uint16_t*, const uint16_t*, int, int, int, int, int, int, hipStream_t);
int launch_paged_encoder_window(const float*, const float*, const int*, void* const*, const int*, const int*, int, int, int,
                                int, int, int, int, hipStream_t);
// single-launch scan over the contiguous caches (attention_fused_naive.hip): 1 = ran, 0 = shape not covered, else error + (rc > 0)
int launch_fused_decode_naive(const float*, const float*, const float*, const int*, float*, int, int, int, void*, size_t,
                              hipStream_t);
int launch_qkt_paged_bf16(const float*, const uint16_t* const*, const int*, float*, int, int, int, hipStream_t);
// fp8 (OCP e4m3) pages with bf16 weights: MLI_ELEM_FP8 of the lean entry points
int launch_latest_paged_fp8(uint8_t* const*, const int*, const uint16_t*, const uint16_t*, const uint16_t*, float*, int, int,
                            int, hipStream_t);
int launch_fill_paged_fp8_embed(const float*, const float*, const int*, uint8_t* const*, const int*, const int*,
                                const uint16_t*, const uint16_t*, int, int, int, int, hipStream_t);
int launch_softmax_v_paged_bf16(const float*, const uint16_t* const*, const int*, float*, int, int, int, void*, size_t,
                                hipStream_t);
// the lean scan's two kernel families behind launch_lean_scan, over the workspace body, each instantiated in one file per page
// element type: one head under a window, with or without sinks (attention_window.hpp: B, S, D, kind, window, n_sink), and
// several heads, grouped or not (attention_heads.hpp: B, S, D, n_heads, n_kv_heads, lg, kind, window, n_sink)
template <class E>
int launch_window_decode(const float*, const void* const*, const int*, float*, int, int, int, ScanKind, int, int, void*, size_t,
                         hipStream_t);
template <class E>
int launch_heads_scan(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, ScanKind, int, int,
                      void*, size_t, hipStream_t);
// ... and the multi-head scans with a position bias per head (attention_alibi.hpp: ..., n_sink, slopes)
template <class E>
int launch_heads_alibi_scan(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, ScanKind, int, int,
                            const float*, void*, size_t, hipStream_t);
// ... and with logit soft-capping (attention_softcap.hpp: ..., n_sink, cap)
template <class E>
int launch_heads_softcap_scan(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, ScanKind, int,
                              int, float, void*, size_t, hipStream_t);
// ... and with a learned sink logit per query head (attention_sink_logits.hpp: ..., n_sink, sink_logits)
template <class E>
int launch_heads_sink_logits_scan(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, ScanKind,
                                  int, int, const float*, void*, size_t, hipStream_t);

// EXTENSION, rotary position embeddings (proj_gemm.hip): the projection and the fills with K and q rotated in the epilogue
int rope_half(int D, int n_heads, const float* table);
int launch_latest_paged_rope(int, void* const*, const int*, const void*, const void*, const void*, float*, int, int, int, int,
                             const float*, hipStream_t);
int launch_fill_paged_rope(int, const float*, const float*, const int*, void* const*, const int*, const int*, const void*,
                           const void*, int, int, int, int, bool, int, int, int, const float*, hipStream_t);

// What every lean paged composition starts with, by page element type (MLI_ELEM_*; bf16 weights for bf16 and fp8 pages):
// fill the n_new_items new rows, then project every non-empty row's last token (k, v appended, q to q_output)
static int launch_fill_and_latest(int elem, void* const* page_table, const int* lengths, const void* wk, const void* wq,
                           const void* wv, const int* new_batch_idx, float* q_output, int n_batch, int n_sequence,
                           int emb_dim, int n_new_items, hipStream_t st) {
    int rc;
    if (elem == MLI_ELEM_FP8) {
        uint8_t* const* pt = reinterpret_cast<uint8_t* const*>(page_table);
        const mli_bf16 *k = static_cast<const mli_bf16*>(wk), *q = static_cast<const mli_bf16*>(wq), *v = static_cast<const mli_bf16*>(wv);
        rc = launch_fill_paged_fp8_embed(nullptr, nullptr, nullptr, pt, new_batch_idx, lengths, k, v, n_batch, n_sequence,
                                         emb_dim, n_new_items, st);
        if (!rc) rc = launch_latest_paged_fp8(pt, lengths, k, q, v, q_output, n_batch, n_sequence, emb_dim, st);
    } else if (elem == MLI_ELEM_BF16) {
        mli_bf16* const* pt = reinterpret_cast<mli_bf16* const*>(page_table);
        const mli_bf16 *k = static_cast<const mli_bf16*>(wk), *q = static_cast<const mli_bf16*>(wq), *v = static_cast<const mli_bf16*>(wv);
        rc = launch_fill_paged_bf16(pt, new_batch_idx, lengths, k, v, n_batch, n_sequence, emb_dim, n_new_items, st);
        if (!rc) rc = launch_latest_paged_bf16(pt, lengths, k, q, v, q_output, n_batch, n_sequence, emb_dim, st);
    } else if (elem == MLI_ELEM_F32) {
        float* const* pt = reinterpret_cast<float* const*>(page_table);
        const float *k = static_cast<const float*>(wk), *q = static_cast<const float*>(wq), *v = static_cast<const float*>(wv);
        rc = launch_fill_paged(pt, new_batch_idx, lengths, k, v, n_batch, n_sequence, emb_dim, n_new_items, st);
        if (!rc) rc = launch_latest_paged(pt, lengths, k, q, v, q_output, n_batch, n_sequence, emb_dim, st);
    } else {
        rc = MLI_ERR_BAD_ARG;
    }
    return rc;
}

// The lean scans' one argument check: which scan (n_heads, n_kv_heads, window, n_sink) is (lean_scan_kind), or
// MLI_ERR_BAD_ARG where the head counts are no grouping or that scan does not take the shape.  One head without a window is
// the plain single-head scan, which judges its shape itself ("not applicable", below): only the element type is held here.
static int lean_scan_args(int B, int S, int D, int n_heads, int n_kv_heads, int window, int n_sink, int elem) {
    if (n_heads < 1 || n_kv_heads < 1 || n_kv_heads > n_heads || n_heads % n_kv_heads != 0) return MLI_ERR_BAD_ARG;
    const ScanKind kind = lean_scan_kind(S, window, n_sink);
    const bool ok = n_kv_heads != n_heads ? gqa_shape_supported(B, S, D, n_heads, n_kv_heads, elem)
                    : kind != kScanPlain  ? window_shape_supported(B, S, D, n_heads, elem)
                    : n_heads > 1         ? heads_lanes_log2(B, S, D, n_heads, elem) >= 0
                                          : elem >= MLI_ELEM_F32 && elem <= MLI_ELEM_FP8;
    return ok ? (int)kind : MLI_ERR_BAD_ARG;
}

int launch_lean_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                     int n_heads, int n_kv_heads, int window, int n_sink, int elem, void* workspace, size_t workspace_bytes,
                     hipStream_t st) {
    const int kind = lean_scan_args(B, S, D, n_heads, n_kv_heads, window, n_sink, elem);
    if (kind < 0) return kind;
    const WsBody body = ws_body(workspace, workspace_bytes);
    if (n_heads > 1) {
        const int lg = heads_lanes_log2(B, S, D, n_heads, elem);
        const auto go = [&](auto e) {
            return launch_heads_scan<decltype(e)>(q, page_table, lengths, out, B, S, D, n_heads, n_kv_heads, lg, (ScanKind)kind,
                                                  window, n_sink, body.ptr, body.bytes, st);
        };
        return elem == MLI_ELEM_BF16 ? go(ElemBF16{}) : go(ElemF32{});
    }
    if (kind != kScanPlain) {
        const auto go = [&](auto e) {
            return launch_window_decode<decltype(e)>(q, page_table, lengths, out, B, S, D, (ScanKind)kind, window, n_sink,
                                                     body.ptr, body.bytes, st);
        };
        return elem == MLI_ELEM_FP8 ? go(ElemFP8{}) : elem == MLI_ELEM_BF16 ? go(ElemBF16{}) : go(ElemF32{});
    }
    // not applicable (rows too wide for the single-pass kernel, or no workspace) is a bad argument: the host layers then
    // take the materialising composition
    return fused_status(launch_fused_decode_elem(elem, q, page_table, lengths, nullptr, out, B, S, D, body.ptr, body.bytes, st, 7));
}

int launch_lean_attention(int elem, void* const* page_table, const int* lengths, const void* wk, const void* wq,
                          const void* wv, const int* new_batch_idx, float* q_output, float* out, int B, int S, int D,
                          int n_new_items, int n_heads, int n_kv_heads, int window, int n_sink, void* workspace,
                          size_t workspace_bytes, hipStream_t st) {
    const int rc = launch_fill_and_latest(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, B, S, D, n_new_items, st);
    if (rc) return rc;
    return launch_lean_scan(q_output, reinterpret_cast<const void* const*>(page_table), lengths, out, B, S, D, n_heads,
                            n_kv_heads, window, n_sink, elem, workspace, workspace_bytes, st);
}

// The fronts of the lean entry points with heads, a window, sinks or grouped K/V heads, one per pair (scan form, fill-first
// form): the pair's own argument rules, then lean_scan_args -- negative is MLI_ERR_BAD_ARG, before anything is launched.
// _heads: fp32 and bf16 pages only, one head included
static int heads_front(int B, int S, int D, int n_heads, int elem) {
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return MLI_ERR_BAD_ARG;
    return lean_scan_args(B, S, D, n_heads, n_heads, 0, 0, elem);
}
// _window (n_sink 0) and _sinks: a window below one is refused; one head takes fp8 pages
static int sinks_front(int B, int S, int D, int n_heads, int window, int n_sink, int elem) {
    if (n_sink < 0 || window < 1) return MLI_ERR_BAD_ARG;
    return lean_scan_args(B, S, D, n_heads, n_heads, window, n_sink, elem);
}
// _gqa: fp32 and bf16 pages only, one head included; a window below one is no window
static int gqa_front(int B, int S, int D, int n_heads, int n_kv_heads, int window, int n_sink, int elem) {
    if ((elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) || n_sink < 0 || S < 1) return MLI_ERR_BAD_ARG;
    return lean_scan_args(B, S, D, n_heads, n_kv_heads, window, n_sink, elem);
}
// _alibi: the _gqa front with two heads at least (the single-head scans have no bias) and the slopes given
static int alibi_front(int B, int S, int D, int n_heads, int n_kv_heads, int window, int n_sink, const float* slopes, int elem) {
    if (n_heads < 2 || slopes == nullptr) return MLI_ERR_BAD_ARG;
    if (!gqa_shape_supported(B, S, D, n_heads, n_kv_heads, elem)) return MLI_ERR_BAD_ARG;   // (holds n_kv_heads and fp8 too)
    return gqa_front(B, S, D, n_heads, n_kv_heads, window, n_sink, elem);
}

// the scan behind the _alibi entry points, after alibi_front (kind = its answer)
static int launch_alibi_scan(int kind, const float* q, const void* const* page_table, const int* lengths, float* out, int B,
                             int S, int D, int n_heads, int n_kv_heads, int window, int n_sink, const float* slopes, int elem,
                             void* workspace, size_t workspace_bytes, hipStream_t st) {
    const WsBody body = ws_body(workspace, workspace_bytes);
    const int lg = heads_lanes_log2(B, S, D, n_heads, elem);
    const auto go = [&](auto e) {
        return launch_heads_alibi_scan<decltype(e)>(q, page_table, lengths, out, B, S, D, n_heads, n_kv_heads, lg, (ScanKind)kind,
                                                    window, n_sink, slopes, body.ptr, body.bytes, st);
    };
    return elem == MLI_ELEM_BF16 ? go(ElemBF16{}) : go(ElemF32{});
}
// _softcap: the _gqa front with two heads at least (the single-head scans have no cap) and a finite cap > 0
static int softcap_front(int B, int S, int D, int n_heads, int n_kv_heads, int window, int n_sink, float cap, int elem) {
    if (n_heads < 2 || !(cap > 0.f) || !std::isfinite(cap)) return MLI_ERR_BAD_ARG;
    if (!gqa_shape_supported(B, S, D, n_heads, n_kv_heads, elem)) return MLI_ERR_BAD_ARG;   // (holds n_kv_heads and fp8 too)
    return gqa_front(B, S, D, n_heads, n_kv_heads, window, n_sink, elem);
}

// the scan behind the _softcap entry points, after softcap_front (kind = its answer)
static int launch_softcap_scan(int kind, const float* q, const void* const* page_table, const int* lengths, float* out, int B,
                               int S, int D, int n_heads, int n_kv_heads, int window, int n_sink, float cap, int elem,
                               void* workspace, size_t workspace_bytes, hipStream_t st) {
    const WsBody body = ws_body(workspace, workspace_bytes);
    const int lg = heads_lanes_log2(B, S, D, n_heads, elem);
    const auto go = [&](auto e) {
        return launch_heads_softcap_scan<decltype(e)>(q, page_table, lengths, out, B, S, D, n_heads, n_kv_heads, lg,
                                                      (ScanKind)kind, window, n_sink, cap, body.ptr, body.bytes, st);
    };
    return elem == MLI_ELEM_BF16 ? go(ElemBF16{}) : go(ElemF32{});
}
// _sink_logits: the _gqa front with two heads at least (the single-head scans have no sink logit), the logits given and no null
// data pointer
static int sink_logits_front(int B, int S, int D, int n_heads, int n_kv_heads, int window, int n_sink, const float* sink_logits,
                             const void* q, const void* page_table, const void* lengths, const void* out, int elem) {
    if (n_heads < 2 || sink_logits == nullptr) return MLI_ERR_BAD_ARG;
    if (!gqa_shape_supported(B, S, D, n_heads, n_kv_heads, elem)) return MLI_ERR_BAD_ARG;   // (holds n_kv_heads and fp8 too)
    if (q == nullptr || page_table == nullptr || lengths == nullptr || out == nullptr) return MLI_ERR_BAD_ARG;
    return gqa_front(B, S, D, n_heads, n_kv_heads, window, n_sink, elem);
}

// the scan behind the _sink_logits entry points, after sink_logits_front (kind = its answer)
static int launch_sink_logits_scan(int kind, const float* q, const void* const* page_table, const int* lengths, float* out, int B,
                                   int S, int D, int n_heads, int n_kv_heads, int window, int n_sink, const float* sink_logits,
                                   int elem, void* workspace, size_t workspace_bytes, hipStream_t st) {
    const WsBody body = ws_body(workspace, workspace_bytes);
    const int lg = heads_lanes_log2(B, S, D, n_heads, elem);
    const auto go = [&](auto e) {
        return launch_heads_sink_logits_scan<decltype(e)>(q, page_table, lengths, out, B, S, D, n_heads, n_kv_heads, lg,
                                                          (ScanKind)kind, window, n_sink, sink_logits, body.ptr, body.bytes, st);
    };
    return elem == MLI_ELEM_BF16 ? go(ElemBF16{}) : go(ElemF32{});
}
// ---- prompt log-probabilities (attention_prompt.hpp) ----------------------------------------------------------------------------
int launch_prompt_sink_logits_scan_elem(const float*, const void* const*, const int*, const int*, const int*, const int*, float*,
                                        int, int, int, int, int, int, int, int, int, int, const float*, int,
                                        hipStream_t);   // attention_prompt.hip
int launch_prompt_project_q(int, const void* const*, const int*, const int*, const int*, const int*, const void*, void*, float*,
                            int, int, int, int, int, int, hipStream_t);   // proj_gemm.hip
int launch_prompt_scan_elem(const float*, const void* const*, const int*, const int*, const int*, const int*, float*, int, int,
                            int, int, int, int, int, int, int, int, int, hipStream_t);   // attention_prompt.hip
int launch_prompt_softcap_scan_elem(const float*, const void* const*, const int*, const int*, const int*, const int*, float*, int,
                                    int, int, int, int, int, int, int, int, int, float, int, hipStream_t);   // attention_prompt.hip
int launch_gemm_nt(const float*, const float*, float*, int, int, int, hipStream_t);
int launch_score_tokens_skipping(const float*, const int*, float*, int*, float*, int, int, int, int, void*);   // decoder_sample.hip

// the token that FOLLOWS every scored position: targets[offset + j] = inp[row, first + j + 1], -1 beyond the sequence and for
// a negative token id (scored as -inf either way).  Every target is kPromptNoRow before this kernel runs, so the rows of a
// skipped segment keep that mark and the scoring leaves them alone: a dense row that belongs to no query is never written.
constexpr int kPromptNoRowByte = 0x80;
constexpr int kPromptNoRow = (int)0x80808080u;
__global__ __launch_bounds__(256) void prompt_targets_kernel(const int* __restrict__ inp, const int* __restrict__ seg_row,
                                                             const int* __restrict__ seg_first, const int* __restrict__ seg_count,
                                                             const int* __restrict__ seg_offset, int* __restrict__ targets,
                                                             int n_seg, int max_count, int n_q, int B, int S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_seg * max_count) return;
    const int seg = i / max_count, j = i % max_count;
    const int cnt = seg_count[seg];
    if (j >= cnt) return;
    const int b = seg_row[seg], first = seg_first[seg], off = seg_offset[seg];
    if (b < 0 || b >= B || first < 0 || (int64_t)first + cnt > S || off < 0 || (int64_t)off + cnt > n_q) return;
    const int s = first + j + 1;
    const int token = s < S ? inp[(int64_t)b * S + s] : -1;
    targets[off + j] = token < 0 ? -1 : token;
}

// scratch of mli_paged_prompt_logprobs: gathered x | q | attention | logits | targets, each region 256-byte aligned
struct PromptScratch {
    size_t gathered, q, attn, logits, targets, total;
};
static PromptScratch prompt_scratch(int n, int D, int V) {
    const auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
    PromptScratch p;
    const size_t row = up((size_t)n * D * sizeof(float));
    p.gathered = 0;
    p.q = row;
    p.attn = 2 * row;
    p.logits = 3 * row;
    p.targets = p.logits + up((size_t)n * V * sizeof(float));
    p.total = p.targets + up((size_t)n * sizeof(int));
    return p;
}

}  // namespace mli

extern "C" {

size_t mli_prompt_logprobs_scratch_bytes(int n_positions, int emb_dim, int n_vocab) {
    if (n_positions <= 0 || emb_dim <= 0 || n_vocab <= 0) return 0;
    return mli::prompt_scratch(n_positions, emb_dim, n_vocab).total;
}

int mli_prompt_project_q(const void* const* page_table, const int* seg_row, const int* seg_first, const int* seg_count,
                         const int* seg_offset, const void* wq, void* gathered, float* q, int n_seg, int max_count, int n_q,
                         int n_batch, int n_sequence, int emb_dim, int elem, void* stream) {
    return mli::launch_prompt_project_q(elem, page_table, seg_row, seg_first, seg_count, seg_offset, wq, gathered, q, n_seg,
                                        max_count, n_q, n_batch, n_sequence, emb_dim, mli::as_stream(stream));
}

static int prompt_logprobs(const void* const* page_table, const int* inp, const void* wq, const float* emb_table,
                              const int* seg_row, const int* seg_first, const int* seg_count, const int* seg_offset,
                              float* token_logprob, int* top_ids, float* top_logprobs, int n_seg, int max_count,
                              int n_positions, int n_batch, int n_sequence, int emb_dim, int n_vocab, int n_heads,
                              int n_kv_heads, int window, int n_sink, int elem, int n_top, void* scratch, size_t scratch_bytes,
                              void* stream, bool capped, float cap, bool sunk = false, const float* sink_logits = nullptr) {
    if (capped && (n_heads < 2 || !(cap > 0.f) || !std::isfinite(cap))) return MLI_ERR_BAD_ARG;
    if (sunk && (n_heads < 2 || sink_logits == nullptr)) return MLI_ERR_BAD_ARG;
    if (n_top < 0 || n_top > MLI_MAX_TOP_LOGPROBS || token_logprob == nullptr ||
        (n_top > 0 && (top_ids == nullptr || top_logprobs == nullptr)))
        return MLI_ERR_BAD_ARG;
    if (n_seg < 0 || window < 0 || n_sink < 0 || n_vocab <= 0 ||
        !mli::prompt_scan_shape_ok(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, elem))
        return MLI_ERR_BAD_ARG;
    if (n_seg == 0) return 0;
    // the list's own limits, the projection's (a segment per y of the gather's grid) and the scan's grid among them: with the
    // shapes, before any pointer is looked at and before the projection is launched
    if (max_count < 1 || max_count > n_sequence || n_positions < 1 || n_seg > 65535) return MLI_ERR_BAD_ARG;
    const int epl = elem == MLI_ELEM_BF16 ? 8 : 4;
    if (!mli::prompt_scan_grid_ok(n_seg, max_count,
                                  mli::prompt_scan_tq(epl, mli::plan_ceil_div(emb_dim / epl, mli::kPlanWave), n_heads > 1)))
        return MLI_ERR_BAD_ARG;
    if (inp == nullptr || wq == nullptr || emb_table == nullptr) return MLI_ERR_BAD_ARG;
    const mli::PromptScratch p = mli::prompt_scratch(n_positions, emb_dim, n_vocab);
    if (scratch == nullptr || scratch_bytes < p.total) return MLI_ERR_WORKSPACE;
    hipStream_t st = mli::as_stream(stream);
    char* base = static_cast<char*>(scratch);
    float* q = reinterpret_cast<float*>(base + p.q);
    float* attn = reinterpret_cast<float*>(base + p.attn);
    float* logits = reinterpret_cast<float*>(base + p.logits);
    int* targets = reinterpret_cast<int*>(base + p.targets);
    int rc = mli::launch_prompt_project_q(elem, page_table, seg_row, seg_first, seg_count, seg_offset, wq, base + p.gathered, q,
                                          n_seg, max_count, n_positions, n_batch, n_sequence, emb_dim, st);
    if (rc) return rc;
    if (sunk)
        rc = mli::launch_prompt_sink_logits_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, attn, n_seg,
                                                      max_count, n_positions, n_batch, n_sequence, emb_dim, n_heads, n_kv_heads,
                                                      window, n_sink, sink_logits, elem, st);
    else if (capped)
        rc = mli::launch_prompt_softcap_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, attn, n_seg, max_count,
                                                  n_positions, n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink,
                                                  cap, elem, st);
    else
        rc = mli::launch_prompt_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, attn, n_seg, max_count,
                                          n_positions, n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, elem,
                                          st);
    if (rc) return rc;
    rc = mli::launch_gemm_nt(attn, emb_table, logits, n_positions, n_vocab, emb_dim, st);
    if (rc) return rc;
    (void)hipMemsetAsync(targets, mli::kPromptNoRowByte, (size_t)n_positions * sizeof(int), st);
    rc = mli::launch_status();   // (the status of the runtime's last call, as after a launch)
    if (rc) return rc;
    hipLaunchKernelGGL(mli::prompt_targets_kernel, dim3(mli::ceil_div_i(n_seg * max_count, 256)), dim3(256), 0, st, inp, seg_row,
                       seg_first, seg_count, seg_offset, targets, n_seg, max_count, n_positions, n_batch, n_sequence);
    rc = mli::launch_status();
    if (rc) return rc;
    return mli::launch_score_tokens_skipping(logits, targets, token_logprob, top_ids, top_logprobs, n_positions, n_vocab, n_top,
                                                mli::kPromptNoRow, stream);
}

int mli_paged_prompt_logprobs(const void* const* page_table, const int* inp, const void* wq, const float* emb_table,
                              const int* seg_row, const int* seg_first, const int* seg_count, const int* seg_offset,
                              float* token_logprob, int* top_ids, float* top_logprobs, int n_seg, int max_count,
                              int n_positions, int n_batch, int n_sequence, int emb_dim, int n_vocab, int n_heads,
                              int n_kv_heads, int window, int n_sink, int elem, int n_top, void* scratch, size_t scratch_bytes,
                              void* stream) {
    return prompt_logprobs(page_table, inp, wq, emb_table, seg_row, seg_first, seg_count, seg_offset, token_logprob, top_ids,
                           top_logprobs, n_seg, max_count, n_positions, n_batch, n_sequence, emb_dim, n_vocab, n_heads, n_kv_heads,
                           window, n_sink, elem, n_top, scratch, scratch_bytes, stream, false, 0.f);
}

int mli_paged_prompt_logprobs_softcap(const void* const* page_table, const int* inp, const void* wq, const float* emb_table,
                                      const int* seg_row, const int* seg_first, const int* seg_count, const int* seg_offset,
                                      float* token_logprob, int* top_ids, float* top_logprobs, int n_seg, int max_count,
                                      int n_positions, int n_batch, int n_sequence, int emb_dim, int n_vocab, int n_heads,
                                      int n_kv_heads, int window, int n_sink, float cap, int elem, int n_top, void* scratch,
                                      size_t scratch_bytes, void* stream) {
    return prompt_logprobs(page_table, inp, wq, emb_table, seg_row, seg_first, seg_count, seg_offset, token_logprob, top_ids,
                           top_logprobs, n_seg, max_count, n_positions, n_batch, n_sequence, emb_dim, n_vocab, n_heads, n_kv_heads,
                           window, n_sink, elem, n_top, scratch, scratch_bytes, stream, true, cap);
}

int mli_paged_prompt_logprobs_sink_logits(const void* const* page_table, const int* inp, const void* wq, const float* emb_table,
                                          const int* seg_row, const int* seg_first, const int* seg_count, const int* seg_offset,
                                          float* token_logprob, int* top_ids, float* top_logprobs, int n_seg, int max_count,
                                          int n_positions, int n_batch, int n_sequence, int emb_dim, int n_vocab, int n_heads,
                                          int n_kv_heads, int window, int n_sink, const float* sink_logits, int elem, int n_top,
                                          void* scratch, size_t scratch_bytes, void* stream) {
    return prompt_logprobs(page_table, inp, wq, emb_table, seg_row, seg_first, seg_count, seg_offset, token_logprob, top_ids,
                           top_logprobs, n_seg, max_count, n_positions, n_batch, n_sequence, emb_dim, n_vocab, n_heads, n_kv_heads,
                           window, n_sink, elem, n_top, scratch, scratch_bytes, stream, false, 0.f, true, sink_logits);
}

int mli_abi_version(void) { return 4; }

int mli_elem_supported(int elem) { return elem == MLI_ELEM_F32 || elem == MLI_ELEM_BF16 || elem == MLI_ELEM_FP8; }

int mli_paged_attention_lean(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                             const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                             int n_sequence, int emb_dim, int n_new_items, int elem_bf16, void* workspace,
                             size_t workspace_bytes, void* stream) {
    if (elem_bf16 < MLI_ELEM_F32 || elem_bf16 > MLI_ELEM_FP8) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_attention(elem_bf16, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                      n_batch, n_sequence, emb_dim, n_new_items, 1, 1, 0, 0, workspace, workspace_bytes,
                                      mli::as_stream(stream));
}

// ---- the lean forms with heads, a window, sinks or grouped K/V heads: a front (above), then the scan, or fill + latest + scan.
// Fill and projection depend on none of n_heads, n_kv_heads, window and n_sink: the pages stay emb_dim wide.  One head
// without a window is mli_decode_scan_paged (phases 7) / mli_paged_attention_lean, n_kv_heads == n_heads the call without
// grouping, n_sink 0 the call without sinks: the same kernels, the same bits, whichever entry point is asked.
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

int mli_decode_scan_paged_heads(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int elem,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (mli::heads_front(n_batch, n_sequence, emb_dim, n_heads, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                 n_heads, 0, 0, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

int mli_paged_attention_lean_heads(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                   const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                   int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int elem,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (mli::heads_front(n_batch, n_sequence, emb_dim, n_heads, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_attention(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                      n_batch, n_sequence, emb_dim, n_new_items, n_heads, n_heads, 0, 0, workspace,
                                      workspace_bytes, mli::as_stream(stream));
}

int mli_decode_scan_paged_window(const float* q_output, const void* const* page_table, const int* lengths,
                                 float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int window,
                                 int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (mli::sinks_front(n_batch, n_sequence, emb_dim, n_heads, window, 0, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                 n_heads, window, 0, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

int mli_paged_attention_lean_window(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                    const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                    int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int window,
                                    int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (mli::sinks_front(n_batch, n_sequence, emb_dim, n_heads, window, 0, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_attention(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                      n_batch, n_sequence, emb_dim, n_new_items, n_heads, n_heads, window, 0, workspace,
                                      workspace_bytes, mli::as_stream(stream));
}

int mli_decode_scan_paged_sinks(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int window,
                                int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (mli::sinks_front(n_batch, n_sequence, emb_dim, n_heads, window, n_sink, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                 n_heads, window, n_sink, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

int mli_paged_attention_lean_sinks(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                   const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                   int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int window,
                                   int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (mli::sinks_front(n_batch, n_sequence, emb_dim, n_heads, window, n_sink, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_attention(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result,
                                      n_batch, n_sequence, emb_dim, n_new_items, n_heads, n_heads, window, n_sink, workspace,
                                      workspace_bytes, mli::as_stream(stream));
}

int mli_decode_scan_paged_gqa(const float* q_output, const void* const* page_table, const int* lengths,
                              float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads,
                              int window, int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (mli::gqa_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                 n_kv_heads, window, n_sink, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

int mli_paged_attention_lean_gqa(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                 const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                 int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                 int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream) {
    if (mli::gqa_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, elem) < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_lean_attention(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result, n_batch,
                                      n_sequence, emb_dim, n_new_items, n_heads, n_kv_heads, window, n_sink, workspace,
                                      workspace_bytes, mli::as_stream(stream));
}

int mli_decode_scan_paged_alibi(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads,
                                int window, int n_sink, const float* slopes, int elem, void* workspace, size_t workspace_bytes,
                                void* stream) {
    const int kind = mli::alibi_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, slopes, elem);
    if (kind < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_alibi_scan(kind, q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                  n_kv_heads, window, n_sink, slopes, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

int mli_paged_attention_lean_alibi(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                   const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                   int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                   int n_sink, const float* slopes, int elem, void* workspace, size_t workspace_bytes,
                                   void* stream) {
    const int kind = mli::alibi_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, slopes, elem);
    if (kind < 0) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    const int rc = mli::launch_fill_and_latest(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, n_batch,
                                               n_sequence, emb_dim, n_new_items, st);
    if (rc) return rc;
    return mli::launch_alibi_scan(kind, q_output, reinterpret_cast<const void* const*>(page_table), lengths, attention_result,
                                  n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, slopes, elem, workspace,
                                  workspace_bytes, st);
}

int mli_alibi_slopes(int n_heads, float* out_host) {
    if (n_heads < 1 || out_host == nullptr) return MLI_ERR_BAD_ARG;
    int n = 1;
    while (2 * n <= n_heads) n *= 2;
    for (int i = 0; i < n; ++i) out_host[i] = (float)std::pow(2.0, -8.0 * (i + 1) / n);
    for (int k = 0; n + k < n_heads; ++k) out_host[n + k] = (float)std::pow(2.0, -4.0 * (2 * k + 1) / n);
    return 0;
}

// ---- EXTENSION: rotary position embeddings ------------------------------------------------------------------------------------
int mli_rope_table(int n_sequence, int head_dim, double theta, float* out_host) {
    if (out_host == nullptr || n_sequence < 1 || head_dim < 2 || head_dim % 2 != 0 || !std::isfinite(theta) || theta <= 0.0)
        return MLI_ERR_BAD_ARG;
    const int half = head_dim / 2;
    for (int i = 0; i < half; ++i) {
        const double inv = std::pow(theta, -2.0 * i / head_dim);
        for (int s = 0; s < n_sequence; ++s) {
            const double ang = s * inv;
            out_host[((size_t)s * half + i) * 2] = (float)std::cos(ang);
            out_host[((size_t)s * half + i) * 2 + 1] = (float)std::sin(ang);
        }
    }
    return 0;
}

int mli_paged_prefill_rope(const float* emb_table, const float* wpe, const int* inp, void* const* page_table, const int* lengths,
                           const int* new_item_indices, const void* wk, const void* wv, int n_batch, int n_sequence, int emb_dim,
                           int n_new_items, int window, int n_sink, int n_heads, const float* rope_table, int elem, void* stream) {
    if (mli::rope_half(emb_dim, n_heads, rope_table) < 0 || window < 0 || n_sink < 0) return MLI_ERR_BAD_ARG;
    if (emb_table == nullptr || wpe == nullptr || inp == nullptr || elem < MLI_ELEM_F32 || elem > MLI_ELEM_FP8) return MLI_ERR_BAD_ARG;
    const bool win = mli::lean_scan_kind(n_sequence, window, n_sink) != mli::kScanPlain;   // else no row has a dead page
    hipStream_t st = mli::as_stream(stream);
    // the form is mli_paged_prefill[_window]'s: the prologue form, or encoder + fill beyond emb_dim 512 (fp8: always the prologue)
    const bool fused = elem == MLI_ELEM_FP8 || mli::prefill_fuses(emb_dim);
    int rc;
    if (fused) {
        rc = mli::launch_fill_paged_rope(elem, emb_table, wpe, inp, page_table, new_item_indices, lengths, wk, wv, n_batch,
                                         n_sequence, emb_dim, n_new_items, win, window, n_sink, n_heads, rope_table, st);
        if (!rc && n_new_items > 0) mli::count_launch(mli::kLfPrefillFused);
        return rc;
    }
    if (n_new_items > 0 && (n_batch <= 0 || n_sequence % mli::kPage != 0 || emb_dim % (elem == MLI_ELEM_BF16 ? 8 : 4) != 0))
        return MLI_ERR_BAD_ARG;   // what the fill refuses, before the encoder is launched
    if (n_new_items > 0) mli::count_launch(mli::kLfPrefillTwoLaunch);
    if (win)
        rc = mli::launch_paged_encoder_window(emb_table, wpe, inp, page_table, lengths, new_item_indices, n_batch, n_sequence,
                                              emb_dim, n_new_items, window, n_sink, elem, st);
    else if (elem == MLI_ELEM_BF16)
        rc = mli_paged_attention_encoder_bf16(emb_table, wpe, inp, reinterpret_cast<mli_bf16* const*>(page_table), lengths,
                                              new_item_indices, n_batch, n_sequence, emb_dim, n_new_items, stream);
    else
        rc = mli_paged_attention_encoder(emb_table, wpe, inp, reinterpret_cast<float* const*>(page_table), lengths,
                                         new_item_indices, n_batch, n_sequence, emb_dim, n_new_items, stream);
    if (rc) return rc;
    return mli::launch_fill_paged_rope(elem, nullptr, nullptr, nullptr, page_table, new_item_indices, lengths, wk, wv, n_batch,
                                       n_sequence, emb_dim, n_new_items, win, window, n_sink, n_heads, rope_table, st);
}

// fill_rope -> latest_rope -> the scan router, unchanged: with slopes the _alibi scan under its front, without them the _gqa
// call's (one head included; one head also on fp8 pages, which the single-head scans take and _gqa has no need to)
int mli_paged_attention_lean_rope(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                  const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                  int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                  int n_sink, const float* slopes, const float* rope_table, int elem, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (mli::rope_half(emb_dim, n_heads, rope_table) < 0) return MLI_ERR_BAD_ARG;
    int kind;
    if (slopes != nullptr)
        kind = mli::alibi_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, slopes, elem);
    else if (elem == MLI_ELEM_FP8 && n_heads == 1 && n_kv_heads == 1 && n_sink >= 0 && n_sequence >= 1)
        kind = mli::lean_scan_args(n_batch, n_sequence, emb_dim, 1, 1, window, n_sink, elem);
    else
        kind = mli::gqa_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, elem);
    if (kind < 0) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    int rc = mli::launch_fill_paged_rope(elem, nullptr, nullptr, nullptr, page_table, new_batch_idx, lengths, wk, wv, n_batch,
                                         n_sequence, emb_dim, n_new_items, false, 0, 0, n_heads, rope_table, st);
    if (!rc)
        rc = mli::launch_latest_paged_rope(elem, page_table, lengths, wk, wq, wv, q_output, n_batch, n_sequence, emb_dim, n_heads,
                                           rope_table, st);
    if (rc) return rc;
    const void* const* pt = reinterpret_cast<const void* const*>(page_table);
    if (slopes != nullptr)
        return mli::launch_alibi_scan(kind, q_output, pt, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                      n_kv_heads, window, n_sink, slopes, elem, workspace, workspace_bytes, st);
    return mli::launch_lean_scan(q_output, pt, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads, n_kv_heads,
                                 window, n_sink, elem, workspace, workspace_bytes, st);
}

// ---- EXTENSION: logit soft-capping (attention_softcap.hpp) ---------------------------------------------------------------------
int mli_decode_scan_paged_softcap(const float* q_output, const void* const* page_table, const int* lengths,
                                  float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads,
                                  int window, int n_sink, float cap, int elem, void* workspace, size_t workspace_bytes,
                                  void* stream) {
    const int kind = mli::softcap_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, cap, elem);
    if (kind < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_softcap_scan(kind, q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, n_heads,
                                    n_kv_heads, window, n_sink, cap, elem, workspace, workspace_bytes, mli::as_stream(stream));
}

// fill -> latest (both rotated where a table is given) -> the capped scan.  Fill and projection never see the cap.
int mli_paged_attention_lean_softcap(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                     const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                     int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                     int n_sink, float cap, const float* rope_table, int elem, void* workspace,
                                     size_t workspace_bytes, void* stream) {
    const int kind = mli::softcap_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, cap, elem);
    if (kind < 0) return MLI_ERR_BAD_ARG;
    if (rope_table != nullptr && mli::rope_half(emb_dim, n_heads, rope_table) < 0) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    int rc;
    if (rope_table != nullptr) {
        rc = mli::launch_fill_paged_rope(elem, nullptr, nullptr, nullptr, page_table, new_batch_idx, lengths, wk, wv, n_batch,
                                         n_sequence, emb_dim, n_new_items, false, 0, 0, n_heads, rope_table, st);
        if (!rc)
            rc = mli::launch_latest_paged_rope(elem, page_table, lengths, wk, wq, wv, q_output, n_batch, n_sequence, emb_dim,
                                               n_heads, rope_table, st);
    } else {
        rc = mli::launch_fill_and_latest(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, n_batch, n_sequence,
                                         emb_dim, n_new_items, st);
    }
    if (rc) return rc;
    return mli::launch_softcap_scan(kind, q_output, reinterpret_cast<const void* const*>(page_table), lengths, attention_result,
                                    n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, cap, elem, workspace,
                                    workspace_bytes, st);
}

// ---- EXTENSION: learned attention-sink logits (attention_sink_logits.hpp) ------------------------------------------------------
int mli_decode_scan_paged_sink_logits(const float* q_output, const void* const* page_table, const int* lengths,
                                      float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads,
                                      int n_kv_heads, int window, int n_sink, const float* sink_logits, int elem, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    const int kind = mli::sink_logits_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, sink_logits,
                                            q_output, page_table, lengths, attention_result, elem);
    if (kind < 0) return MLI_ERR_BAD_ARG;
    return mli::launch_sink_logits_scan(kind, q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim,
                                        n_heads, n_kv_heads, window, n_sink, sink_logits, elem, workspace, workspace_bytes,
                                        mli::as_stream(stream));
}

// fill -> latest (both rotated where a table is given) -> the scan with sink logits.  Fill and projection never see them.
int mli_paged_attention_lean_sink_logits(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                         const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                         int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads,
                                         int window, int n_sink, const float* sink_logits, const float* rope_table, int elem,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    const int kind = mli::sink_logits_front(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, sink_logits,
                                            q_output, page_table, lengths, attention_result, elem);
    if (kind < 0 || wk == nullptr || wq == nullptr || wv == nullptr) return MLI_ERR_BAD_ARG;
    if (rope_table != nullptr && mli::rope_half(emb_dim, n_heads, rope_table) < 0) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    int rc;
    if (rope_table != nullptr) {
        rc = mli::launch_fill_paged_rope(elem, nullptr, nullptr, nullptr, page_table, new_batch_idx, lengths, wk, wv, n_batch,
                                         n_sequence, emb_dim, n_new_items, false, 0, 0, n_heads, rope_table, st);
        if (!rc)
            rc = mli::launch_latest_paged_rope(elem, page_table, lengths, wk, wq, wv, q_output, n_batch, n_sequence, emb_dim,
                                               n_heads, rope_table, st);
    } else {
        rc = mli::launch_fill_and_latest(elem, page_table, lengths, wk, wq, wv, new_batch_idx, q_output, n_batch, n_sequence,
                                         emb_dim, n_new_items, st);
    }
    if (rc) return rc;
    return mli::launch_sink_logits_scan(kind, q_output, reinterpret_cast<const void* const*>(page_table), lengths,
                                        attention_result, n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink,
                                        sink_logits, elem, workspace, workspace_bytes, st);
}

int mli_get_latest_k_q_v_paged_lean(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                    const void* wv, float* q_output, int n_batch, int n_sequence, int emb_dim, int elem,
                                    void* stream) {
    hipStream_t st = mli::as_stream(stream);
    if (elem == MLI_ELEM_FP8)
        return mli::launch_latest_paged_fp8(reinterpret_cast<uint8_t* const*>(page_table), lengths, static_cast<const mli_bf16*>(wk),
                                            static_cast<const mli_bf16*>(wq), static_cast<const mli_bf16*>(wv), q_output, n_batch,
                                            n_sequence, emb_dim, st);
    if (elem == MLI_ELEM_BF16)
        return mli::launch_latest_paged_bf16(reinterpret_cast<mli_bf16* const*>(page_table), lengths, static_cast<const mli_bf16*>(wk),
                                             static_cast<const mli_bf16*>(wq), static_cast<const mli_bf16*>(wv), q_output, n_batch,
                                             n_sequence, emb_dim, st);
    if (elem == MLI_ELEM_F32)
        return mli::launch_latest_paged(reinterpret_cast<float* const*>(page_table), lengths, static_cast<const float*>(wk),
                                        static_cast<const float*>(wq), static_cast<const float*>(wv), q_output, n_batch,
                                        n_sequence, emb_dim, st);
    return MLI_ERR_BAD_ARG;
}

int mli_self_attention_lean(const float* inp_embedding, const int* lengths, const float* wk, const float* wq,
                            const float* wv, const int* new_batch_idx, float* kt_cache, float* v_cache, float* q_output,
                            float* attention_result, int n_batch, int n_sequence, int input_dim, int output_dim,
                            int n_new_items, void* workspace, size_t workspace_bytes, void* stream) {
    { const mli::WsBody body = mli::ws_body(workspace, workspace_bytes); workspace = body.ptr; workspace_bytes = body.bytes; }
    hipStream_t st = mli::as_stream(stream);
    int rc = mli::launch_fill_naive(inp_embedding, new_batch_idx, lengths, wk, wv, kt_cache, v_cache, n_batch,
                                    n_sequence, input_dim, output_dim, n_new_items, st);
    if (rc) return rc;
    rc = mli::launch_latest_naive(inp_embedding, lengths, wk, wq, wv, kt_cache, v_cache, q_output, n_batch,
                                  n_sequence, input_dim, output_dim, st);
    if (rc) return rc;
    const int fused = mli::launch_fused_decode_naive(q_output, kt_cache, v_cache, lengths, attention_result, n_batch,
                                                     n_sequence, output_dim, workspace, workspace_bytes, st);
    if (fused == 1) return 0;
    // shapes the single-launch scan does not cover (dims not multiples of 4, no workspace): the caller takes the
    // materialising composition -- the projection it has just run is idempotent
    if (fused == 0) return MLI_ERR_BAD_ARG;
    return fused < 0 ? fused : fused - 1;
}

int mli_paged_decode_step(void* const* page_table, int* lengths, const void* wk, const void* wq, const void* wv,
                          const float* emb_table, const float* wpe_table, float* q_output, float* attention_result,
                          int* decoder_result, int n_batch, int n_sequence, int emb_dim, int n_vocab,
                          int n_decoder_results, int i_decoder, int elem_bf16, void* workspace, size_t workspace_bytes,
                          void* decoder_scratch, size_t decoder_scratch_bytes, void* stream) {
    const int rc = mli_paged_attention_lean(page_table, lengths, wk, wq, wv, /*new_batch_idx=*/nullptr, q_output,
                                            attention_result, n_batch, n_sequence, emb_dim, /*n_new_items=*/0, elem_bf16,
                                            workspace, workspace_bytes, stream);
    if (rc) return rc;
    return mli_paged_decoder_fused(attention_result, emb_table, wpe_table, page_table, lengths, decoder_result, n_batch,
                                   n_vocab, n_sequence, emb_dim, n_decoder_results, i_decoder, elem_bf16, decoder_scratch,
                                   decoder_scratch_bytes, stream);
}

int mli_decode_step(float* inp_embedding, int* lengths, const float* wk, const float* wq, const float* wv,
                    const float* emb_table, const float* wpe_table, float* kt_cache, float* v_cache, float* q_output,
                    float* qkt_output, float* attention_result, int* decoder_result, int n_batch, int n_sequence,
                    int emb_dim, int n_vocab, void* workspace, size_t workspace_bytes, void* decoder_scratch,
                    size_t decoder_scratch_bytes, void* stream) {
    int rc = mli_self_attention_lean(inp_embedding, lengths, wk, wq, wv, /*new_batch_idx=*/nullptr, kt_cache, v_cache,
                                     q_output, attention_result, n_batch, n_sequence, emb_dim, emb_dim, /*n_new_items=*/0,
                                     workspace, workspace_bytes, stream);
    if (rc == MLI_ERR_BAD_ARG)  // a shape the single-launch scan does not cover: scores and probabilities through qkt_output
        rc = mli_inference_self_attention(inp_embedding, lengths, wk, wq, wv, /*new_batch_idx=*/nullptr, kt_cache, v_cache,
                                          q_output, qkt_output, attention_result, n_batch, n_sequence, emb_dim, emb_dim,
                                          /*n_new_items=*/0, workspace, workspace_bytes, stream);
    if (rc) return rc;
    return mli_decoder_fused(attention_result, emb_table, wpe_table, inp_embedding, lengths, decoder_result, n_batch,
                             n_vocab, n_sequence, emb_dim, decoder_scratch, decoder_scratch_bytes, stream);
}

int mli_paged_prefill(const float* emb_table, const float* wpe, const int* inp, void* const* page_table,
                      const int* lengths, const int* new_item_indices, const void* wk, const void* wv, int n_batch,
                      int n_sequence, int emb_dim, int n_new_items, int elem_bf16, void* stream) {
    if (emb_table == nullptr || wpe == nullptr || inp == nullptr) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    if (elem_bf16 < MLI_ELEM_F32 || elem_bf16 > MLI_ELEM_FP8) return MLI_ERR_BAD_ARG;
    if (n_new_items > 0)
        mli::count_launch(elem_bf16 == MLI_ELEM_FP8 || mli::prefill_fuses(emb_dim) ? mli::kLfPrefillFused : mli::kLfPrefillTwoLaunch);
    if (elem_bf16 == MLI_ELEM_FP8)
        return mli::launch_fill_paged_fp8_embed(emb_table, wpe, inp, reinterpret_cast<uint8_t* const*>(page_table),
                                                new_item_indices, lengths, static_cast<const mli_bf16*>(wk),
                                                static_cast<const mli_bf16*>(wv), n_batch, n_sequence, emb_dim, n_new_items, st);
    // The prologue form reads emb_table and wpe (fp32, 8 bytes per element) in EVERY column tile instead of the 2- or
    // 4-byte x element: worth one launch boundary and the x round trip while there are few column tiles, a loss beyond
    // (emb_dim 2048: 64 column tiles, 199 us against 154 + 14 us for encoder + fill; emb_dim 256: 8 tiles, a gain) -- so
    // wide models take the two launches.  Pages are bit-identical either way (tested).
    if (!mli::prefill_fuses(emb_dim)) {
        int rc = elem_bf16 ? mli_paged_attention_encoder_bf16(emb_table, wpe, inp, reinterpret_cast<mli_bf16* const*>(page_table),
                                                              lengths, new_item_indices, n_batch, n_sequence, emb_dim,
                                                              n_new_items, stream)
                           : mli_paged_attention_encoder(emb_table, wpe, inp, reinterpret_cast<float* const*>(page_table),
                                                         lengths, new_item_indices, n_batch, n_sequence, emb_dim, n_new_items,
                                                         stream);
        if (rc) return rc;
        return elem_bf16 ? mli_fill_new_k_v_cache_paged_bf16(reinterpret_cast<mli_bf16* const*>(page_table), new_item_indices,
                                                             lengths, static_cast<const mli_bf16*>(wk),
                                                             static_cast<const mli_bf16*>(wv), n_batch, n_sequence, emb_dim,
                                                             n_new_items, stream)
                         : mli_fill_new_k_v_cache_paged(reinterpret_cast<float* const*>(page_table), new_item_indices, lengths,
                                                        static_cast<const float*>(wk), static_cast<const float*>(wv), n_batch,
                                                        n_sequence, emb_dim, n_new_items, stream);
    }
    if (elem_bf16)
        return mli::launch_fill_paged_bf16_embed(emb_table, wpe, inp, reinterpret_cast<mli_bf16* const*>(page_table),
                                                 new_item_indices, lengths, static_cast<const mli_bf16*>(wk),
                                                 static_cast<const mli_bf16*>(wv), n_batch, n_sequence, emb_dim,
                                                 n_new_items, st);
    return mli::launch_fill_paged_embed(emb_table, wpe, inp, reinterpret_cast<float* const*>(page_table), new_item_indices,
                                        lengths, static_cast<const float*>(wk), static_cast<const float*>(wv), n_batch,
                                        n_sequence, emb_dim, n_new_items, st);
}

int mli_paged_prefill_window(const float* emb_table, const float* wpe, const int* inp, void* const* page_table,
                             const int* lengths, const int* new_item_indices, const void* wk, const void* wv, int n_batch,
                             int n_sequence, int emb_dim, int n_new_items, int window, int n_sink, int elem, void* stream) {
    if (window < 0 || n_sink < 0) return MLI_ERR_BAD_ARG;
    if (mli::lean_scan_kind(n_sequence, window, n_sink) == mli::kScanPlain)   // no row has a dead page
        return mli_paged_prefill(emb_table, wpe, inp, page_table, lengths, new_item_indices, wk, wv, n_batch, n_sequence,
                                 emb_dim, n_new_items, elem, stream);
    if (emb_table == nullptr || wpe == nullptr || inp == nullptr) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    if (elem < MLI_ELEM_F32 || elem > MLI_ELEM_FP8) return MLI_ERR_BAD_ARG;
    const mli_bf16 *k16 = static_cast<const mli_bf16*>(wk), *v16 = static_cast<const mli_bf16*>(wv);
    if (n_new_items > 0)
        mli::count_launch(elem == MLI_ELEM_FP8 || mli::prefill_fuses(emb_dim) ? mli::kLfPrefillFused : mli::kLfPrefillTwoLaunch);
    if (elem == MLI_ELEM_FP8)
        return mli::launch_fill_paged_fp8_window_embed(emb_table, wpe, inp, reinterpret_cast<uint8_t* const*>(page_table),
                                                       new_item_indices, lengths, k16, v16, n_batch, n_sequence, emb_dim,
                                                       n_new_items, window, n_sink, st);
    // the form is mli_paged_prefill's: the prologue form, or encoder + fill beyond emb_dim 512
    if (!mli::prefill_fuses(emb_dim)) {
        const int rc = mli::launch_paged_encoder_window(emb_table, wpe, inp, page_table, lengths, new_item_indices, n_batch,
                                                        n_sequence, emb_dim, n_new_items, window, n_sink, elem, st);
        if (rc) return rc;
        return elem ? mli::launch_fill_paged_bf16_window(reinterpret_cast<mli_bf16* const*>(page_table), new_item_indices,
                                                         lengths, k16, v16, n_batch, n_sequence, emb_dim, n_new_items, window,
                                                         n_sink, st)
                    : mli::launch_fill_paged_window_embed(nullptr, nullptr, nullptr, reinterpret_cast<float* const*>(page_table),
                                                          new_item_indices, lengths, static_cast<const float*>(wk),
                                                          static_cast<const float*>(wv), n_batch, n_sequence, emb_dim,
                                                          n_new_items, window, n_sink, st);
    }
    if (elem)
        return mli::launch_fill_paged_bf16_window_embed(emb_table, wpe, inp, reinterpret_cast<mli_bf16* const*>(page_table),
                                                        new_item_indices, lengths, k16, v16, n_batch, n_sequence, emb_dim,
                                                        n_new_items, window, n_sink, st);
    return mli::launch_fill_paged_window_embed(emb_table, wpe, inp, reinterpret_cast<float* const*>(page_table),
                                               new_item_indices, lengths, static_cast<const float*>(wk),
                                               static_cast<const float*>(wv), n_batch, n_sequence, emb_dim, n_new_items,
                                               window, n_sink, st);
}

int mli_graph_begin_capture(void* stream) {
    if (stream == nullptr) return MLI_ERR_BAD_ARG;  // the legacy default stream cannot be captured
    return (int)hipStreamBeginCapture(mli::as_stream(stream), hipStreamCaptureModeThreadLocal);
}

int mli_graph_end_capture(void* stream, void** graph_exec_out) {
    if (stream == nullptr || graph_exec_out == nullptr) return MLI_ERR_BAD_ARG;
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamEndCapture(mli::as_stream(stream), &graph);
    if (e != hipSuccess) return (int)e;
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) return (int)e;
    *graph_exec_out = exec;
    return 0;
}

int mli_stream_wait_stream(void* waiter, void* signaller) {
    // events are cheap to create and may be destroyed as soon as both calls have been issued: the runtime keeps what it
    // needs until the work has passed (eager), or has already turned it into a graph edge (capture)
    hipEvent_t ev = nullptr;
    hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
    if (e != hipSuccess) return (int)e;
    e = hipEventRecord(ev, mli::as_stream(signaller));
    if (e == hipSuccess) e = hipStreamWaitEvent(mli::as_stream(waiter), ev, 0);
    (void)hipEventDestroy(ev);
    return (int)e;
}

int mli_graph_launch(void* graph_exec, void* stream) {
    if (graph_exec == nullptr) return MLI_ERR_BAD_ARG;
    return (int)hipGraphLaunch(reinterpret_cast<hipGraphExec_t>(graph_exec), mli::as_stream(stream));
}

int mli_graph_destroy(void* graph_exec) {
    if (graph_exec == nullptr) return 0;
    return (int)hipGraphExecDestroy(reinterpret_cast<hipGraphExec_t>(graph_exec));
}

int mli_paged_attention_bf16(mli_bf16* const* page_table, const int* lengths, const mli_bf16* wk, const mli_bf16* wq,
                             const mli_bf16* wv, const int* new_batch_idx, float* q_output, float* qkt_output,
                             float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_new_items,
                             void* workspace, size_t workspace_bytes, void* stream) {
    { const mli::WsBody body = mli::ws_body(workspace, workspace_bytes); workspace = body.ptr; workspace_bytes = body.bytes; }
    hipStream_t st = mli::as_stream(stream);
    int rc = mli::launch_fill_paged_bf16(page_table, new_batch_idx, lengths, wk, wv, n_batch, n_sequence, emb_dim,
                                         n_new_items, st);
    if (rc) return rc;
    rc = mli::launch_latest_paged_bf16(page_table, lengths, wk, wq, wv, q_output, n_batch, n_sequence, emb_dim, st);
    if (rc) return rc;
    const int fused = mli::launch_fused_decode_bf16(q_output, page_table, lengths, qkt_output, attention_result, n_batch,
                                                    n_sequence, emb_dim, workspace, workspace_bytes, st);
    if (fused == 1) return 0;
    if (fused != 0) return fused < 0 ? fused : fused - 1;
    return mli::launch_scores_softmax_v_paged_bf16(q_output, page_table, lengths, qkt_output, attention_result,
                                                   n_batch, n_sequence, emb_dim, workspace, workspace_bytes, st);
}

int mli_inference_self_attention(const float* inp_embedding, const int* lengths, const float* wk, const float* wq,
                                 const float* wv, const int* new_batch_idx, float* kt_cache, float* v_cache,
                                 float* q_output, float* qkt_output, float* attention_result, int n_batch,
                                 int n_sequence, int input_dim, int output_dim, int n_new_items, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    { const mli::WsBody body = mli::ws_body(workspace, workspace_bytes); workspace = body.ptr; workspace_bytes = body.bytes; }
    hipStream_t st = mli::as_stream(stream);
    int rc = mli::launch_fill_naive(inp_embedding, new_batch_idx, lengths, wk, wv, kt_cache, v_cache, n_batch,
                                    n_sequence, input_dim, output_dim, n_new_items, st);
    if (rc) return rc;
    rc = mli::launch_latest_naive(inp_embedding, lengths, wk, wq, wv, kt_cache, v_cache, q_output, n_batch,
                                  n_sequence, input_dim, output_dim, st);
    if (rc) return rc;
    return mli::launch_scores_softmax_v_naive(q_output, kt_cache, v_cache, lengths, qkt_output, attention_result,
                                              n_batch, n_sequence, output_dim, workspace, workspace_bytes, st);
}

int mli_paged_attention(float* const* page_table, const int* lengths, const float* wk, const float* wq,
                        const float* wv, const int* new_batch_idx, float* q_output, float* qkt_output,
                        float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_new_items,
                        void* workspace, size_t workspace_bytes, void* stream) {
    { const mli::WsBody body = mli::ws_body(workspace, workspace_bytes); workspace = body.ptr; workspace_bytes = body.bytes; }
    hipStream_t st = mli::as_stream(stream);
    int rc = mli::launch_fill_paged(page_table, new_batch_idx, lengths, wk, wv, n_batch, n_sequence, emb_dim,
                                    n_new_items, st);
    if (rc) return rc;
    rc = mli::launch_latest_paged(page_table, lengths, wk, wq, wv, q_output, n_batch, n_sequence, emb_dim, st);
    if (rc) return rc;
    const int fused = mli::launch_fused_decode_f32(q_output, page_table, lengths, qkt_output, attention_result, n_batch,
                                                   n_sequence, emb_dim, workspace, workspace_bytes, st);
    if (fused == 1) return 0;
    if (fused != 0) return fused < 0 ? fused : fused - 1;
    return mli::launch_scores_softmax_v_paged(q_output, page_table, lengths, qkt_output, attention_result, n_batch,
                                              n_sequence, emb_dim, workspace, workspace_bytes, st);
}

}  // extern "C"
