/*
 * mli_kernels.h -- C ABI of libmli_hip.so, the MI355X (gfx950) implementation of the
 * single-block self-attention decode path of xyg-coder/min_llm_inference.
 *
 * This header is the drop-in boundary.  The reference has no FFI layer: its boundary is
 * the C++ `launch_*` free functions declared in the headers under include/kernels/ (reference paths
 * below are relative to the reference repository root).  Every entry point here is the
 * POD form of exactly one of those functions; the C++ adapters with the reference's own
 * signatures live in min_llm_inference_amd/host/src/launchers.cpp and only unpack
 * Tensor shapes before calling into this ABI.
 *
 * Conventions
 *   - all pointers are DEVICE pointers unless the name ends in _host;
 *   - every buffer is caller-owned and pre-allocated; no entry point allocates, frees
 *     or synchronises (all are legal inside hipGraph capture);
 *   - `stream` is a hipStream_t passed as void*; NULL = the legacy default stream,
 *     which is what the reference launches on;
 *   - return value: 0 on success, a positive hipError_t when a launch failed, or
 *     MLI_ERR_BAD_ARG when a shape precondition the reference asserts on is violated;
 *   - indices are int32 as in the reference, offsets are computed in 64 bit;
 *   - page layout (reference include/utils.h:32-60): a page block holds
 *     PAGE_BLOCK_SIZE=16 tokens, float offset inside a block =
 *     (s % 16) * 3 * emb_dim + seg * emb_dim + d, seg 0 = input embedding, 1 = K, 2 = V;
 *     page table entry index = b * (n_sequence / 16) + s / 16.
 */
#ifndef MLI_KERNELS_H
#define MLI_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLI_PAGE_BLOCK_SIZE 16
#define MLI_EMPTY_ROW_TOKEN_ID (-1)
#define MLI_EOF_TOKEN_ID 1023
#define MLI_ERR_BAD_ARG (-22)
#define MLI_ERR_WORKSPACE (-12)

/* ABI version; bumped whenever a signature below changes. */
int mli_abi_version(void);

/* Page / weight element types of the lean entry points (their `elem` argument; the reference is fp32 only):
 *   MLI_ELEM_F32   float pages and weights -- the reference's types
 *   MLI_ELEM_BF16  EXTENSION: bfloat16 pages and weights (BASELINE config 4)
 *   MLI_ELEM_FP8   EXTENSION, opt-in: OCP e4m3 pages (x, K and V segments; one byte per element under the same layout
 *                  rule), bfloat16 weights; q, scores, softmax and every accumulation stay fp32
 * mli_elem_supported: 1 when this build implements the element type, 0 otherwise. */
#define MLI_ELEM_F32 0
#define MLI_ELEM_BF16 1
#define MLI_ELEM_FP8 2
int mli_elem_supported(int elem);

/* Bytes of device scratch the split-sequence kernels need for a problem of this size
 * (softmax_v / softmax_v_paged / paged_attention / inference_self_attention): per-chunk softmax statistics,
 * the split-sequence partial sums, and -- in a fixed 64 KiB region at the front, so that calls of different shapes can
 * share one buffer -- one arrival counter per batch row for the lean single-pass scan.  Never 0 for a valid shape.
 * The owner zero-fills that region ONCE after allocating the buffer (mli_attention_workspace_init); every entry point
 * leaves the counters zero on return, so nothing is re-initialised per call (nor under graph replay).  One workspace
 * serves one stream at a time. */
size_t mli_attention_workspace_bytes(int n_batch, int n_sequence, int dim);
/* Zero-fills the arrival counters at the front of a freshly allocated workspace (the first 64 KiB; a buffer that was
 * allocated zero-filled needs no call).  Stream-ordered; once per allocation, not per call. */
int mli_attention_workspace_init(void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Contiguous ("naive") KV-cache path.
 *   inp_embedding [n_batch, n_sequence, input_dim]   kt_cache [n_batch, output_dim, n_sequence]
 *   v_cache       [n_batch, n_sequence, output_dim]  wk/wq/wv [input_dim, output_dim]
 * ---------------------------------------------------------------------------------- */

/* replaces launch_fill_new_kt_v_cache  (include/kernels/self_attention_inference_optimized.h:5-8,
 * src/kernels/self_attention_inference_optimized.cu:303-323).  No-op when n_new_items == 0. */
int mli_fill_new_kt_v_cache(const float* inp_embedding, const int* new_batch_idx, const int* lengths,
                            const float* wk, const float* wv, float* kt_cache, float* v_cache,
                            int n_batch, int n_sequence, int input_dim, int output_dim,
                            int n_new_items, void* stream);

/* replaces launch_get_latest_kt_q_v  (…optimized.h:11-15, …optimized.cu:325-343).
 * Rows with lengths[b]==0 are left untouched (q_output included). */
int mli_get_latest_kt_q_v(const float* inp_embedding, const int* lengths,
                          const float* wk, const float* wq, const float* wv,
                          float* kt_cache, float* v_cache, float* q_output,
                          int n_batch, int n_sequence, int input_dim, int output_dim, void* stream);

/* replaces launch_qkt  (…optimized.h:17-19, …optimized.cu:345-358).
 * qkt_output[b, s] for s >= lengths[b] is not written. */
int mli_qkt(const float* q_output, const float* kt_cache, const int* lengths, float* qkt_output,
            int n_batch, int n_sequence, int dim, void* stream);

/* replaces launch_softmax_in_place_with_lengths  (…optimized.h:21-22, …optimized.cu:360-368).
 * Requires n_sequence % 4 == 0 (reference device assert, …optimized.cu:195).  Writes the whole
 * row: probabilities for s < lengths[b], 0 for the tail. */
int mli_softmax_in_place_with_lengths(float* qkt_output, const int* lengths,
                                      int n_batch, int n_sequence, void* stream);

/* replaces launch_softmax_v  (…optimized.h:24-26, …optimized.cu:370-383).
 * workspace may be NULL only when n_sequence <= 64 (single chunk: nothing is staged). */
int mli_softmax_v(const float* softmax_result, const float* v_cache, const int* lengths,
                  float* attention_result, int n_batch, int n_sequence, int output_dim,
                  void* workspace, size_t workspace_bytes, void* stream);

/* replaces inference_self_attention  (…optimized.h:28-48, …optimized.cu:282-301):
 * fill -> latest -> qkt -> softmax -> softmax_v on one stream. */
int mli_inference_self_attention(const float* inp_embedding, const int* lengths,
                                 const float* wk, const float* wq, const float* wv,
                                 const int* new_batch_idx, float* kt_cache, float* v_cache,
                                 float* q_output, float* qkt_output, float* attention_result,
                                 int n_batch, int n_sequence, int input_dim, int output_dim,
                                 int n_new_items, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Paged KV-cache path.  page_table is float*[n_batch][n_sequence/16] of device pointers.
 * Requires n_sequence % 16 == 0 and emb_dim % 4 == 0 (reference asserts,
 * src/kernels/paged_attention.cu:105-107, src/kernels/paged_attention_cublas.cu:212).
 * ---------------------------------------------------------------------------------- */

/* replaces launch_fill_new_k_v_cache_paged_attention (include/kernels/paged_attention.h:28-30,
 * src/kernels/paged_attention.cu:96-115) AND launch_fill_new_k_v_cache_paged_attention_warp_tiling
 * (paged_attention.h:65-67, src/kernels/paged_attention_cublas.cu:225-246): one MFMA kernel. */
int mli_fill_new_k_v_cache_paged(float* const* page_table, const int* new_batch_idx, const int* lengths,
                                 const float* wk, const float* wv,
                                 int n_batch, int n_sequence, int emb_dim, int n_new_items, void* stream);

/* replaces launch_get_latest_k_q_v_paged_attention (paged_attention.h:32-35, paged_attention.cu:188-199)
 * AND launch_get_latest_k_q_v_paged_attention_cublas (paged_attention.h:57-63,
 * paged_attention_cublas.cu:76-99: gather + 3 cublasSgemm + scatter) as one gather-GEMM-scatter kernel. */
int mli_get_latest_k_q_v_paged(float* const* page_table, const int* lengths,
                               const float* wk, const float* wq, const float* wv, float* q_output,
                               int n_batch, int n_sequence, int emb_dim, void* stream);

/* replaces launch_qkt_paged_attention (paged_attention.h:37-39, paged_attention.cu:270-280). */
/* mli_qkt_paged[_bf16] and mli_qkt stage the row's q in LDS: emb_dim beyond what 64 KiB hold beside the item's page pointers
 * (16360 with a small batch; mli_qkt: dim <= 15344) is MLI_ERR_BAD_ARG before anything is launched.
 * mli_decode_scan_contiguous takes emb_dim <= 13052 for the same reason. */
int mli_qkt_paged(const float* q_output, const float* const* page_table, const int* lengths,
                  float* qkt_output, int n_batch, int n_sequence, int emb_dim, void* stream);

/* replaces launch_softmax_v_paged_attention (paged_attention.h:41-43, paged_attention.cu:333-345). */
int mli_softmax_v_paged(const float* softmax_result, const float* const* page_table, const int* lengths,
                        float* attention_result, int n_batch, int n_sequence, int emb_dim,
                        void* workspace, size_t workspace_bytes, void* stream);

/* replaces paged_attention (paged_attention.h:17-25, paged_attention.cu:358-377) and
 * paged_attention_with_cublas (paged_attention.h:46-54, paged_attention_cublas.cu:260-280).
 * On return q_output, qkt_output (probabilities, zero tail) and attention_result hold what the
 * reference's five launches leave there. */
int mli_paged_attention(float* const* page_table, const int* lengths,
                        const float* wk, const float* wq, const float* wv, const int* new_batch_idx,
                        float* q_output, float* qkt_output, float* attention_result,
                        int n_batch, int n_sequence, int emb_dim, int n_new_items,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * bfloat16 paged path (BASELINE.json config 4).  EXTENSION: the reference is fp32 only, so these entry
 * points have no reference counterpart; they are the fp32 paged entry points above with 16-bit pages
 * (same layout rule, elements are bf16) and bf16 weights.  q_output, qkt_output, attention_result and
 * every accumulation stay fp32.  Requires emb_dim % 8 == 0.  mli_bf16 = raw bfloat16 bits.
 * ---------------------------------------------------------------------------------- */
typedef uint16_t mli_bf16;

int mli_fill_new_k_v_cache_paged_bf16(mli_bf16* const* page_table, const int* new_batch_idx, const int* lengths,
                                      const mli_bf16* wk, const mli_bf16* wv,
                                      int n_batch, int n_sequence, int emb_dim, int n_new_items, void* stream);

int mli_get_latest_k_q_v_paged_bf16(mli_bf16* const* page_table, const int* lengths,
                                    const mli_bf16* wk, const mli_bf16* wq, const mli_bf16* wv, float* q_output,
                                    int n_batch, int n_sequence, int emb_dim, void* stream);

int mli_qkt_paged_bf16(const float* q_output, const mli_bf16* const* page_table, const int* lengths,
                       float* qkt_output, int n_batch, int n_sequence, int emb_dim, void* stream);

int mli_softmax_v_paged_bf16(const float* softmax_result, const mli_bf16* const* page_table, const int* lengths,
                             float* attention_result, int n_batch, int n_sequence, int emb_dim,
                             void* workspace, size_t workspace_bytes, void* stream);

int mli_paged_attention_bf16(mli_bf16* const* page_table, const int* lengths,
                             const mli_bf16* wk, const mli_bf16* wq, const mli_bf16* wv, const int* new_batch_idx,
                             float* q_output, float* qkt_output, float* attention_result,
                             int n_batch, int n_sequence, int emb_dim, int n_new_items,
                             void* workspace, size_t workspace_bytes, void* stream);

/* fp32 embedding tables in, bf16 input embedding written into segment 0 of the page */
int mli_paged_attention_encoder_bf16(const float* emb_table, const float* wpe, const int* inp,
                                     mli_bf16* const* page_table, const int* lengths, const int* new_item_indices,
                                     int n_batch, int n_sequence, int emb_dim, int n_new_items, void* stream);

int mli_paged_decoder_multi_rounds_bf16(const float* batch_result, const float* emb_table, float* emb_score,
                                        const float* wpe_table, mli_bf16* const* page_table, int* lengths,
                                        int* decoder_result, int n_batch, int n_vocab, int n_sequence, int emb_dim,
                                        int n_decoder_results, int i_decoder, void* stream);

/* LEAN paged composition -- what PagedAttention*Layer::forward runs.  The reference's paged_attention also leaves the
 * softmax probabilities in its qkt_output scratch (paged_attention.h:17-25), which nothing downstream reads
 * (src/layers.cpp:84-100 passes attention_result on, qkt_output stays in the layer).  This form computes the same
 * attention_result (bit-identical to mli_paged_attention[_bf16]) without materialising scores or probabilities:
 * fill (n_new_items rows) -> latest -> single-pass scan whose chunk results are merged inside the scan launch by the
 * workgroup that completes a row.  elem_bf16 selects the page / weight element type (0 = float, 1 = mli_bf16). */
int mli_paged_attention_lean(void* const* page_table, const int* lengths,
                             const void* wk, const void* wq, const void* wv, const int* new_batch_idx,
                             float* q_output, float* attention_result,
                             int n_batch, int n_sequence, int emb_dim, int n_new_items, int elem_bf16,
                             void* workspace, size_t workspace_bytes, void* stream);

/* EXTENSION: MULTI-HEAD attention for the lean paged composition and its scan.  n_heads = H >= 1, head_dim = hd =
 * emb_dim / H; head h owns columns [h * hd, (h + 1) * hd) of q_output and of the K and V segments of every page slot:
 *     x[h][s] = sum_{d < hd} q[b, h*hd + d] * K[b, s, h*hd + d] / sqrtf(hd),  p[h][.] = softmax over s < lengths[b],
 *     attention_result[b, h*hd + d] = sum_s p[h][s] * V[b, s, h*hd + d]
 * (no output projection: the model has none).  Rows of length 0 give zeros, slots >= lengths[b] are never multiplied, a
 * null page reads as zeros.  Fill, projection, page layout and q_output do not depend on H.  H == 1 is exactly
 * mli_paged_attention_lean / mli_decode_scan_paged(phases 7): same kernels, same bits.  For H > 1 -- one scan launch, no
 * scores materialised, chunked grid, in-kernel merge per head; of the mli_tune keys "chunk_tokens", "nt_loads" and
 * "scan_row_order" apply -- the supported shapes are: emb_dim % H == 0; hd in {32, 64, 128, 256}; elem MLI_ELEM_F32 with
 * emb_dim <= 512 or MLI_ELEM_BF16 with emb_dim <= 1024; n_sequence % 16 == 0; n_batch <= 16384.  Everything else (and
 * MLI_ELEM_FP8 with any H) is MLI_ERR_BAD_ARG, decided before anything is launched.
 *
 * Workspace: mli_attention_heads_workspace_bytes >= mli_attention_workspace_bytes of the same shape (equal at H == 1), so
 * one buffer serves both kinds of call; 0 for an unsupported combination.  Same layout rule (the 64 KiB counter region in
 * front, zeroed once by mli_attention_workspace_init, zero again after every call); too small: MLI_ERR_WORKSPACE. */
size_t mli_attention_heads_workspace_bytes(int n_batch, int n_sequence, int dim, int n_heads);

/* The multi-head scan on its own: q_output from the projection in, attention_result out. */
int mli_decode_scan_paged_heads(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads,
                                int elem, void* workspace, size_t workspace_bytes, void* stream);

/* mli_paged_attention_lean with n_heads heads: fill (n_new_items rows) -> latest -> multi-head scan. */
int mli_paged_attention_lean_heads(void* const* page_table, const int* lengths,
                                   const void* wk, const void* wq, const void* wv, const int* new_batch_idx,
                                   float* q_output, float* attention_result,
                                   int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int elem,
                                   void* workspace, size_t workspace_bytes, void* stream);

/* EXTENSION: SLIDING-WINDOW attention for the lean paged composition and its scan.  window = W >= 1; for row b with
 * L = min(lengths[b], n_sequence) and lo = max(0, L - W) the row attends slots s in [lo, L) -- its newest W tokens, the
 * newest one (slot L - 1) always among them -- with the scores scaled as without a window (1 / sqrtf(emb_dim) with one
 * head, 1 / sqrtf(head_dim) per head).  L == 0 gives zeros; W == 1 gives the fp32 value of V's row L - 1 bit for bit.
 * No byte of a slot outside [lo, L) influences the result: slots >= L and slots < lo of the first live page are never
 * multiplied, and the page-table entries of the pages wholly below lo (index < lo / 16) are never read -- they may be
 * null or stale.  Fill, projection, page layout and q_output do not depend on W.
 * W >= n_sequence is "no window": the call IS mli_decode_scan_paged(phases 7) / mli_paged_attention_lean, or the _heads
 * forms for n_heads > 1 -- same kernels, same bits.  For W < n_sequence -- one scan launch, chunked grid sized by the
 * min(n_sequence, 16 * (ceil(W / 16) + 1)) tokens a windowed row can span, in-kernel merge; of the mli_tune keys
 * "chunk_tokens", "nt_loads" and "scan_row_order" apply -- the supported shapes are: n_heads == 1: what the lean chunked
 * scan takes (n_sequence % 16 == 0; MLI_ELEM_F32 to emb_dim 2048, MLI_ELEM_BF16 to 4096, MLI_ELEM_FP8 with emb_dim % 16
 * == 0 to 2048) with n_batch <= 16384; n_heads > 1: what mli_decode_scan_paged_heads takes.  Everything else, window < 1
 * and n_heads < 1 are MLI_ERR_BAD_ARG, decided before anything is launched.
 * Workspace: mli_attention_workspace_bytes (n_heads == 1) / mli_attention_heads_workspace_bytes of the same
 * (n_batch, n_sequence, emb_dim, n_heads): one buffer serves windowed and plain calls; same layout and counter rule. */
int mli_decode_scan_paged_window(const float* q_output, const void* const* page_table, const int* lengths,
                                 float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads,
                                 int window, int elem, void* workspace, size_t workspace_bytes, void* stream);

/* mli_paged_attention_lean[_heads] with a window: fill (n_new_items rows) -> latest -> windowed scan. */
int mli_paged_attention_lean_window(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                    const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                    int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int window,
                                    int elem, void* workspace, size_t workspace_bytes, void* stream);

/* EXTENSION: ATTENTION SINKS beside the sliding window.  n_sink = K >= 0, window = W >= 1; for row b with
 * L = min(lengths[b], n_sequence) and lo = max(0, L - W) the row attends the slots s < L with s < K or s >= lo -- its first
 * K tokens and its newest W (W is not reduced by K); a row with lo <= K attends all of [0, L).  Scores are scaled as without
 * sinks; L == 0 gives zeros.  No byte of a slot outside the attended set influences the result: the gap slots [K, lo) and
 * the slots >= L are never multiplied, not even inside a page they share with attended slots, and the page-table entries
 * of the pages wholly inside the gap (ceil(K / 16) <= index < lo / 16) are never read -- they may be null or stale.  Fill,
 * projection, page layout and q_output depend neither on W nor on K.
 * Hand-offs, before anything else, same kernels and same bits: K == 0 IS the _window call; K + W >= n_sequence or
 * W >= n_sequence (no row can have a gap) IS mli_decode_scan_paged(phases 7) / mli_paged_attention_lean, or the _heads forms
 * for n_heads > 1.  Otherwise one scan launch, chunked grid sized by the min(n_sequence, 16 * (ceil(K / 16) + ceil(W / 16)
 * + 1)) tokens a row's two page runs can span, in-kernel merge; supported shapes, mli_tune keys and the workspace are
 * mli_decode_scan_paged_window's.  K < 0, W < 1 and n_heads < 1 are MLI_ERR_BAD_ARG, decided before anything is launched. */
int mli_decode_scan_paged_sinks(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int window,
                                int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream);

/* mli_paged_attention_lean_window with sinks: fill (n_new_items rows) -> latest -> sink-windowed scan. */
int mli_paged_attention_lean_sinks(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                   const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                   int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int window,
                                   int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream);

/* EXTENSION: GROUPED-QUERY ATTENTION for the multi-head scan.  n_kv_heads = Hkv K/V heads serve n_heads = H query heads,
 * 1 <= Hkv <= H, H % Hkv == 0, g = H / Hkv (any integer; Hkv = 1 is multi-query attention), hd = emb_dim / H.  Query head h
 * owns columns [h * hd, (h + 1) * hd) of q_output and attention_result, as with mli_decode_scan_paged_heads, and attends
 * K/V head h / g, which owns columns [(h / g) * hd, (h / g + 1) * hd) of the K and the V segment of every page slot; the
 * columns >= Hkv * hd of those segments are never read (they may hold anything).  Scores are scaled by 1 / sqrtf(hd).  The
 * result is that of the _sinks call with H heads on pages whose K / V column block h is a copy of block h / g, bit for bit.
 * Page layout, fill, projection and q_output do not depend on Hkv: wk / wv keep their [emb_dim, emb_dim] shape and only
 * their first Hkv * hd output columns matter.  window <= 0 or >= n_sequence: no window; n_sink = 0: no sinks; the attended
 * slots, the zero row for L == 0 and the never-read gap are mli_decode_scan_paged_sinks's.
 * Hand-off, before anything else, same kernels and same bits: n_kv_heads == n_heads IS the _sinks call (n_heads = 1
 * included).  Otherwise one scan launch with the grid, item size, mli_tune keys and workspace
 * (mli_attention_heads_workspace_bytes(n_batch, n_sequence, emb_dim, n_heads)) of H heads; the K / V bytes read fall by g.
 * elem = MLI_ELEM_F32 or MLI_ELEM_BF16.  MLI_ERR_BAD_ARG, decided before anything is launched: another elem, Hkv < 1,
 * Hkv > H, H % Hkv != 0, n_sink < 0, and every shape the _heads / _window entry points refuse.  MLI_ERR_WORKSPACE: a shape
 * of several items per row without the workspace, as for _heads. */
int mli_decode_scan_paged_gqa(const float* q_output, const void* const* page_table, const int* lengths,
                              float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads,
                              int window, int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream);

/* mli_paged_attention_lean_sinks with grouped K/V heads: fill (n_new_items rows) -> latest -> the scan above. */
int mli_paged_attention_lean_gqa(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                 const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                 int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                 int n_sink, int elem, void* workspace, size_t workspace_bytes, void* stream);

/* EXTENSION: ALiBi, A LINEAR POSITION BIAS PER QUERY HEAD, for the multi-head scan (the alibi_slopes argument of other serving
 * stacks' paged attention; the BLOOM / MPT / Baichuan family).  slopes: n_heads fp32 values in DEVICE memory, one per query
 * head, finite, of any sign.  For row b with L = min(lengths[b], n_sequence), query head h, g = n_heads / n_kv_heads and an
 * attended slot s:
 *     x[h][s] = (q_h . K_{h/g}[s]) / sqrtf(head_dim) + slopes[h] * (s - (L - 1))
 * s is the token's ABSOLUTE slot in the row -- not its position in the page, the item, or the virtual row of sink pages and
 * window pages: the gap under sinks counts towards the distance.  The slope is the QUERY head's: under grouping the g heads of
 * a group read the same K/V and carry different slopes.  The bias is 0 at the newest token and, with positive slopes, <= 0
 * everywhere (fp32 scores stay small where the probability mass is).  The attended set for (window, n_sink), the softmax, p . V,
 * the zero row for L == 0 and the never-read dead slots, gap slots and gap pages are mli_decode_scan_paged_gqa's.  Slopes all
 * 0.0f give the bits of that call; L == 1, and a one-slot window without sinks, give V's row L - 1 bit for bit.
 * One scan launch ("scan_heads_alibi"), the grid, item size, mli_tune keys and workspace
 * (mli_attention_heads_workspace_bytes(n_batch, n_sequence, emb_dim, n_heads): one buffer serves plain and ALiBi calls) of
 * the _gqa call.  Shapes: what that call takes with n_heads >= 2 -- head_dim 32, 64, 128 or 256, fp32 pages to emb_dim 512,
 * bf16 pages to 1024; n_kv_heads == n_heads: no grouping.  MLI_ERR_BAD_ARG, decided before anything is launched: n_heads == 1
 * (the single-head scans have no bias), fp8 pages, a null slopes, and every argument the _gqa call refuses.
 * MLI_ERR_WORKSPACE as there. */
int mli_decode_scan_paged_alibi(const float* q_output, const void* const* page_table, const int* lengths,
                                float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads,
                                int window, int n_sink, const float* slopes, int elem, void* workspace, size_t workspace_bytes,
                                void* stream);

/* mli_paged_attention_lean_gqa with the bias: fill (n_new_items rows) -> latest -> the scan above.  Fill and projection never
 * see the slopes. */
int mli_paged_attention_lean_alibi(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                   const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                   int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                   int n_sink, const float* slopes, int elem, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* The standard ALiBi slopes of n_heads heads, written to out_host (HOST memory, n_heads floats; a host function, no GPU).  With
 * n = 2^floor(log2 n_heads): out[i] = (float)pow(2, -8 (i + 1) / n) for i < n; for n_heads > n the remaining n_heads - n are
 * (float)pow(2, -4 (2 k + 1) / n), k = 0 ..., every other slope of the 2 n series.  n_heads < 1 or a null pointer:
 * MLI_ERR_BAD_ARG. */
int mli_alibi_slopes(int n_heads, float* out_host);

/* EXTENSION: ROTARY POSITION EMBEDDINGS (RoPE; the Llama / Mistral / Qwen / Gemma / Phi family) in the paged projection and the
 * paged fills.  The columns of q and K are grouped in heads as for the scans: n_heads = H, hd = emb_dim / H, K/V head blocks
 * at the same column offsets whatever n_kv_heads is.  The pairing is the INTERLEAVED one (GPT-J, Meta's Llama): inside every
 * head, columns 2i and 2i + 1 form pair i, 0 <= i < hd / 2.  For the token at absolute slot s of its row, the GEMM's fp32
 * accumulators a = y[2i], b = y[2i + 1] and (c, sn) = rope_table[s][i] give
 *     y'[2i] = a c - b sn        y'[2i + 1] = b c + a sn
 * computed in fp32 in the GEMM's epilogue (one product rounding, one fma rounding), BEFORE the one rounding of K to the page's
 * element type; q stays fp32; V and the x segment are untouched.  s is the absolute slot in the row: L - 1 for the decode
 * projection, the token's own slot for the fills -- under the flat row list too, and under a window the slot, not the live
 * index.  Windows, sinks and page release never renumber positions (the convention of the ALiBi bias).  The scans do not
 * change: a row's K is stored rotated by its slot and q is rotated by L - 1, so q . K depends on the distance alone.  wpe is
 * still added by the prefill; a RoPE model passes zeros.
 * rope_table: [n_sequence][hd / 2] pairs of fp32 (cos, sin) in DEVICE memory, 8-byte aligned, supplied by the caller -- the
 * scaled variants (linear, NTK, YaRN, Llama-3) are just another table; a table of all (1, 0) gives the bytes of the entry
 * point without the rotation in the whole pool and in q_output.  A table rather than sincosf in the kernel: fp32 range
 * reduction at angles of thousands of radians, determinism, and the scaled variants.
 * Kernels: the ROPE instantiations of the tiled MFMA GEMMs (every form their launchers select in the paged modes; the table is
 * an argument of those instantiations alone).  The latency-shaped panel kernel and the LDS-DMA projection have no such switch
 * yet: with a table their shapes take the tiled kernels.  Launch families "gemm_f32_rope" / "gemm_bf16_rope" are counted
 * beside the family of the form that ran; the mli_tune keys of the un-rotated entry points apply.
 * Shapes: what the un-rotated entry points take, with emb_dim % n_heads == 0 and hd even.  MLI_ERR_BAD_ARG, decided before
 * anything is launched: a null rope_table, n_heads < 1, emb_dim % n_heads != 0, an odd hd, and everything the un-rotated
 * call refuses.  No contiguous-cache form. */

/* The standard table, written to out_host (HOST memory, n_sequence * head_dim floats; a host function, no GPU), in double:
 * inv = pow(theta, -2.0 i / head_dim), ang = s * inv, out[s][i] = ((float)cos(ang), (float)sin(ang)).  MLI_ERR_BAD_ARG: a null
 * pointer, n_sequence < 1, head_dim odd or < 2, theta not finite or <= 0. */
int mli_rope_table(int n_sequence, int head_dim, double theta, float* out_host);

/* mli_get_latest_k_q_v_paged_lean with the rotation: k (rotated, then rounded) and v appended to the page, q (rotated) to
 * q_output, of every non-empty row's last token, slot L - 1. */
int mli_get_latest_k_q_v_paged_rope(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                    float* q_output, int n_batch, int n_sequence, int emb_dim, int n_heads,
                                    const float* rope_table, int elem, void* stream);

/* mli_fill_new_k_v_cache_paged[_bf16] (and its fp8 form) with the rotation, reading x from the pages: K of every token of the
 * n_new_items new rows, rotated by the token's slot; elem = MLI_ELEM_*. */
int mli_fill_new_k_v_cache_paged_rope(void* const* page_table, const int* new_batch_idx, const int* lengths, const void* wk,
                                      const void* wv, int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads,
                                      const float* rope_table, int elem, void* stream);

/* mli_paged_prefill_window's contract with rotated K: the prologue form and the two-launch form by mli_tune "prefill_fused",
 * the flat list and the per-row grid by "fill_compact"; window == 0 (or no row with a dead page): no window. */
int mli_paged_prefill_rope(const float* emb_table, const float* wpe, const int* inp, void* const* page_table, const int* lengths,
                           const int* new_item_indices, const void* wk, const void* wv, int n_batch, int n_sequence, int emb_dim,
                           int n_new_items, int window, int n_sink, int n_heads, const float* rope_table, int elem, void* stream);

/* mli_paged_attention_lean_alibi with the rotation: fill_rope (n_new_items rows) -> latest_rope -> the existing scan router,
 * unchanged.  slopes may be null, meaning no bias: the call then takes mli_paged_attention_lean_gqa's scans and rules, one
 * head included -- and one head on fp8 pages, which the single-head scans take.  With slopes the rules are the _alibi call's.
 * Additionally MLI_ERR_BAD_ARG as above. */
int mli_paged_attention_lean_rope(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                  const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                  int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                  int n_sink, const float* slopes, const float* rope_table, int elem, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* EXTENSION: ATTENTION LOGIT SOFT-CAPPING for the multi-head scan (the logits_soft_cap / attn_logit_softcapping argument of
 * other serving stacks' paged attention; Gemma 2, Grok-1).  cap: one finite fp32 value > 0 per call, a HOST value.  For row b
 * with L = min(lengths[b], n_sequence), query head h, g = n_heads / n_kv_heads and an attended slot s:
 *     x[h][s] = cap * tanh( ((q_h . K_{h/g}[s]) / sqrtf(head_dim)) / cap )
 * The cap is applied to the SCALED score, before the mask and the maximum; a masked slot stays excluded (it never becomes a
 * finite score of -cap).  The attended set for (window, n_sink), the softmax, p . V, the zero row for L == 0 and the never-read
 * dead slots, gap slots and gap pages are mli_decode_scan_paged_gqa's.  There is no cap that gives back the bits of that call;
 * L == 1, and a one-slot window without sinks, give V's row L - 1 bit for bit whatever the cap.  tanh is evaluated in fp32 to
 * about 3.5 * 2^-24 RELATIVE to the score, however small the score is beside the cap.
 * One scan launch ("scan_heads_softcap"), the grid, item size, mli_tune keys and workspace
 * (mli_attention_heads_workspace_bytes(n_batch, n_sequence, emb_dim, n_heads): one buffer serves plain and capped calls) of
 * the _gqa call.  Shapes: what that call takes with n_heads >= 2 -- head_dim 32, 64, 128 or 256, fp32 pages to emb_dim 512,
 * bf16 pages to 1024; n_kv_heads == n_heads: no grouping.  MLI_ERR_BAD_ARG, decided before anything is launched: n_heads == 1
 * (the single-head scans have no cap), fp8 pages, cap <= 0, NaN or infinite, and every argument the _gqa call refuses.
 * MLI_ERR_WORKSPACE as there.  Not combined with ALiBi (no published model uses both; the order of bias and cap would be an
 * invention): there is no slopes argument. */
int mli_decode_scan_paged_softcap(const float* q_output, const void* const* page_table, const int* lengths,
                                  float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads,
                                  int window, int n_sink, float cap, int elem, void* workspace, size_t workspace_bytes,
                                  void* stream);

/* mli_paged_attention_lean_gqa with the cap: fill (n_new_items rows) -> latest -> the scan above.  rope_table: null, or the
 * table of mli_paged_attention_lean_rope (then fill and latest are that call's: K and q rotated; Gemma 2 uses both).  Fill and
 * projection never see the cap.  MLI_ERR_BAD_ARG as above and, with a table, as mli_paged_attention_lean_rope. */
int mli_paged_attention_lean_softcap(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                     const int* new_batch_idx, float* q_output, float* attention_result, int n_batch,
                                     int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads, int window,
                                     int n_sink, float cap, const float* rope_table, int elem, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* EXTENSION: LEARNED ATTENTION-SINK LOGITS for the multi-head scan (the per-head `sinks` parameter of the gpt-oss attention
 * block; z = 0 for every head is the "off-by-one" / "quiet" softmax).  sink_logits: n_heads fp32 values in DEVICE memory, each
 * finite or -inf.  For row b with L = min(lengths[b], n_sequence) >= 1, query head h, g = n_heads / n_kv_heads, the attended set
 * A of the call's form (plain, window, window + n_sink tokens), x[s] = (q_h . K_{h/g}[s]) / sqrtf(head_dim) and z = sink_logits[h]:
 *     m     = max( max_{s in A} x[s], z )
 *     out_h = sum_{s in A} exp(x[s] - m) V_{h/g}[s]  /  ( sum_{s in A} exp(x[s] - m) + exp(z - m) )
 * z takes part in head h's softmax as one more logit WITHOUT a value row: its probability mass is dropped.  It is the QUERY
 * head's logit (the heads of a K/V group have different ones), it is not scaled by 1 / sqrt(head_dim), no window masks it, and it
 * counts ONCE per (row, head) however the row is split.  It is NOT n_sink, which keeps the first tokens of a row attended; the two
 * are used together.  z = -inf: no sink.  Anchors: all logits -inf give the BITS of mli_decode_scan_paged_gqa; a logit of -1e30
 * in head h gives that call's bits in head h's columns; a logit of +1e30 gives exactly 0.0f there on every non-empty row, without
 * NaN or inf (the maximum takes the sink in before any exponential).  +inf and NaN are outside the contract (the values live in
 * device memory; mli_engine_set_sink_logits refuses them).  L == 0 gives the zero row; dead slots, gap slots and gap pages are
 * never read, as in the _gqa call.
 * One scan launch ("scan_heads_sink_logits"), the grid, item size, mli_tune keys and workspace
 * (mli_attention_heads_workspace_bytes(n_batch, n_sequence, emb_dim, n_heads)) of the _gqa call.  Shapes: what that call takes
 * with n_heads >= 2.  MLI_ERR_BAD_ARG, decided before anything is launched: n_heads == 1, fp8 pages, a bad head count, an
 * unsupported shape, a negative n_sink, a null sink_logits or data pointer.  MLI_ERR_WORKSPACE as there.  Not combined with ALiBi
 * or soft-capping (no model defines that): there is no slopes and no cap argument. */
int mli_decode_scan_paged_sink_logits(const float* q_output, const void* const* page_table, const int* lengths,
                                      float* attention_result, int n_batch, int n_sequence, int emb_dim, int n_heads,
                                      int n_kv_heads, int window, int n_sink, const float* sink_logits, int elem, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* mli_paged_attention_lean_gqa with the sink logits: fill (n_new_items rows) -> latest -> the scan above.  rope_table: null, or
 * the table of mli_paged_attention_lean_rope (then fill and latest are that call's: K and q rotated; gpt-oss uses both).  Fill
 * and projection never see the logits.  MLI_ERR_BAD_ARG as above, for a null weight pointer and, with a table, as
 * mli_paged_attention_lean_rope. */
int mli_paged_attention_lean_sink_logits(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                         const void* wv, const int* new_batch_idx, float* q_output, float* attention_result,
                                         int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads, int n_kv_heads,
                                         int window, int n_sink, const float* sink_logits, const float* rope_table, int elem,
                                         void* workspace, size_t workspace_bytes, void* stream);

/* The decode projection of mli_paged_attention_lean on its own (q, k, v of every non-empty row's last token; k, v appended to
 * the page, q to q_output) for any page element type: elem = MLI_ELEM_*.  For fp32 / bf16 pages it is
 * mli_get_latest_k_q_v_paged[_bf16]; fp8 pages have no other entry point for it.  (bench.py times it apart from the scan.) */
int mli_get_latest_k_q_v_paged_lean(void* const* page_table, const int* lengths, const void* wk, const void* wq,
                                    const void* wv, float* q_output, int n_batch, int n_sequence, int emb_dim, int elem,
                                    void* stream);

/* LEAN contiguous composition -- what SelfAttentionLayer::forward runs: inference_self_attention
 * (self_attention_inference_optimized.h:22-25) without its qkt_output scratch (nothing downstream reads it,
 * src/layers.cpp:41-56).  fill (n_new_items rows) -> latest -> ONE scan launch: a workgroup scores 256 tokens of a row
 * from the K^T tile, keeps exp(score - chunk max) in LDS, accumulates it over the V tile, and the workgroup that
 * completes a row merges its chunks (attention_fused_naive.hip).  attention_result differs from
 * mli_inference_self_attention's by fp32 rounding of the merge only.  output_dim and n_sequence must be multiples of 4
 * and the caches 16-byte aligned (the scan reads them in 16-byte pieces; input_dim is free); otherwise MLI_ERR_BAD_ARG
 * after the projection has run (it is idempotent) and the caller takes mli_inference_self_attention. */
int mli_self_attention_lean(const float* inp_embedding, const int* lengths,
                            const float* wk, const float* wq, const float* wv, const int* new_batch_idx,
                            float* kt_cache, float* v_cache, float* q_output, float* attention_result,
                            int n_batch, int n_sequence, int input_dim, int output_dim, int n_new_items,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The scan launch of mli_self_attention_lean on its own: q_output from mli_get_latest_kt_q_v in, attention_result out. */
int mli_decode_scan_contiguous(const float* q_output, const float* kt_cache, const float* v_cache, const int* lengths,
                               float* attention_result, int n_batch, int n_sequence, int emb_dim,
                               void* workspace, size_t workspace_bytes, void* stream);

/* The single-pass scan the paged compositions run after the projection (scores + masked softmax + softmax.V in
 * one visit per page; what A10 -> A4 -> A11 of SURVEY 8(a) compute together).  Inputs: q_output from
 * mli_get_latest_k_q_v_paged[_bf16]; outputs: qkt_output (probabilities, zero tail) and attention_result.
 * elem_bf16 selects the page element type; phases: 1 = scan kernel only, 2 = combine kernel only, 3 = both
 * (1 and 2 exist so the two launches can be timed apart); + 4 = lean mode: qkt_output is neither read nor written
 * (may be NULL) and the scan merges every row's chunks itself, so 5 = 7 = the whole job in ONE launch (6 = nothing;
 * with mli_tune("scan_merge", 0) the merge stays a second, slimmer launch and 5 / 6 time the two apart).  Rows of up to two 16-byte lane loads (fp32 <= 512,
 * bf16 <= 1024) give every wave whole pages; wider rows (fp32 <= 2048, bf16 <= 4096) are split across the four
 * waves of a workgroup; MLI_ELEM_FP8 (lean phases only) takes rows of up to two lane loads (<= 2048).  Returns
 * MLI_ERR_BAD_ARG beyond that, in every phase, before anything is launched: use the separate entry points then.
 * n_batch is not bounded by the 16384 arrival counters: with more rows the lean form keeps the merge in a second, slimmer
 * launch (as under mli_tune("scan_merge", 0)), touches no counter and gives the same bits; the multi-head, window, sink
 * and grouped entry points refuse n_batch > 16384 instead.  n_sequence is bounded by the LDS the merge statistics are staged
 * in -- 8 bytes per 64 tokens of n_sequence beside the item's page pointers, within the 64 KiB a launch gets less 512 bytes
 * for the kernels' static part: n_sequence <= 519936 at items of 64 tokens, 519680 at items of 128 (under a window: 8 bytes
 * per item of the span, the same figures) -- and is MLI_ERR_BAD_ARG beyond that, in every phase and from the window and sink
 * entry points alike, before anything is launched. */
int mli_decode_scan_paged(const float* q_output, const void* const* page_table, const int* lengths,
                          float* qkt_output, float* attention_result, int n_batch, int n_sequence, int emb_dim,
                          int elem_bf16, int phases, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Encoder / decoder head (needed for InferenceModel::forward).
 * ---------------------------------------------------------------------------------- */

/* replaces launch_inference_optimized_encoder_kernel (include/kernels/encoder.h:16-19,
 * src/kernels/encoder.cu:80-92). */
int mli_inference_optimized_encoder(const float* emb_table, const float* wpe, const int* inp,
                                    float* inp_embedding, const int* lengths, const int* new_item_indices,
                                    int n_batch, int n_sequence, int emb_dim, int n_new_items, void* stream);

/* replaces launch_paged_attention_encoder_kernel (encoder.h:22-25, encoder.cu:134-147). */
int mli_paged_attention_encoder(const float* emb_table, const float* wpe, const int* inp,
                                float* const* page_table, const int* lengths, const int* new_item_indices,
                                int n_batch, int n_sequence, int emb_dim, int n_new_items, void* stream);

/* replaces launch_decoder (include/kernels/decoder.h:19-23, src/kernels/decoder.cu:94-111):
 * emb_score = batch_result . emb_table^T, per-row argmax, lengths update, next embedding write. */
int mli_decoder(const float* batch_result, const float* emb_table, float* emb_score, const float* wpe_table,
                float* inp_embedding, int* lengths, int* decoder_result,
                int n_batch, int n_vocab, int n_sequence, int emb_dim, void* stream);

/* replaces launch_paged_attention_decoder_multi_rounds and
 * launch_paged_attention_cublas_decoder_multi_rounds (decoder.h:26-37, decoder.cu:207-255). */
int mli_paged_decoder_multi_rounds(const float* batch_result, const float* emb_table, float* emb_score,
                                   const float* wpe_table, float* const* page_table, int* lengths,
                                   int* decoder_result, int n_batch, int n_vocab, int n_sequence, int emb_dim,
                                   int n_decoder_results, int i_decoder, void* stream);

/* Decoder head with the argmax as the logits GEMM's EPILOGUE: emb_score[n_batch, n_vocab] is
 * never materialised.  Every 64-column tile of the product leaves one (max, lowest index of the max) pair per row in
 * `scratch` (mli_decoder_scratch_bytes), a one-wave-per-row kernel picks the row's token from those pairs, updates the
 * length and writes the next input embedding.  Tokens, lengths and embeddings are identical to mli_decoder /
 * mli_paged_decoder_multi_rounds[_bf16] (same fp32 products, same argmax order: larger value, then lower index) --
 * those stay for callers that want emb_score (the reference's decoder tests compare it).  What *DecoderLayer::forward
 * runs.  Replaces launch_decoder / launch_paged_attention[_cublas]_decoder_multi_rounds (decoder.h:19-37). */
size_t mli_decoder_scratch_bytes(int n_batch, int n_vocab);
int mli_decoder_fused(const float* batch_result, const float* emb_table, const float* wpe_table,
                      float* inp_embedding, int* lengths, int* decoder_result,
                      int n_batch, int n_vocab, int n_sequence, int emb_dim,
                      void* scratch, size_t scratch_bytes, void* stream);
int mli_paged_decoder_fused(const float* batch_result, const float* emb_table, const float* wpe_table,
                            void* const* page_table, int* lengths, int* decoder_result,
                            int n_batch, int n_vocab, int n_sequence, int emb_dim,
                            int n_decoder_results, int i_decoder, int elem_bf16,
                            void* scratch, size_t scratch_bytes, void* stream);

/* EXTENSION: sampled decoder head.  Per batch row b the parameters are device arrays [n_batch]
 * (structure of arrays): temperature T (f32), top_k K (i32), top_p P (f32), seed (i64, read as a 64-bit pattern).
 * The token is drawn at position L = lengths[b]:
 *   - T == 0: the greedy token, bit-identical to mli_[paged_]decoder_fused on the same logits (K and P ignored);
 *   - otherwise, over the finite logits x: keep x >= the K-th largest (K == 0: all), then x >= t_p, the largest kept
 *     value whose softmax(x / T) mass over the kept values >= it is at least P (P == 1: all); the token is the argmax of
 *     x / T + g over that set (ties: lower index), g = -log(-log(u)), u = ((w >> 9) + 0.5f) * 2^-23 (exact, in (0, 1)),
 *     w = Philox4x32-10(counter (v >> 2, L, 0, 0), key (seed low word, seed high word))[v & 3].
 *   - no finite logit: the greedy head's token for that case (-1); empty rows (L == 0) as in the greedy heads.
 * The draw depends on (logits, T, K, P, seed, L) only and is run-to-run deterministic.
 * Out-of-domain device values never fault: T < 0 or NaN decodes greedily, K < 0 acts as 0, P > 1 or NaN acts as 1,
 * P <= 0 keeps only the largest value (ties included).
 *
 * mli_sample_scratch_bytes: device scratch mli_sample_tokens needs (0: none; scratch may then be NULL).
 * mli_sample_tokens: token pick only, logits [n_batch, n_vocab] -> tokens [n_batch]; lengths are read, never written.
 * mli_decoder_sampled / mli_paged_decoder_sampled: the plain logits GEMM into the front of `scratch`
 *   (mli_decoder_sampled_scratch_bytes: the fp32 logits [n_batch, n_vocab] and the pick's own scratch), the pick, then
 *   what mli_[paged_]decoder_fused does with the token: decoder_result, lengths, next input embedding (contiguous or
 *   paged fp32 / bf16 / fp8, `elem`). */
size_t mli_sample_scratch_bytes(int n_batch, int n_vocab);
int mli_sample_tokens(const float* logits, const float* temperature, const int* top_k, const float* top_p,
                      const int64_t* seed, const int* lengths, int* tokens, int n_batch, int n_vocab,
                      void* scratch, size_t scratch_bytes, void* stream);
size_t mli_decoder_sampled_scratch_bytes(int n_batch, int n_vocab);
int mli_decoder_sampled(const float* batch_result, const float* emb_table, const float* wpe_table,
                        float* inp_embedding, int* lengths, int* decoder_result,
                        int n_batch, int n_vocab, int n_sequence, int emb_dim,
                        const float* temperature, const int* top_k, const float* top_p, const int64_t* seed,
                        void* scratch, size_t scratch_bytes, void* stream);
int mli_paged_decoder_sampled(const float* batch_result, const float* emb_table, const float* wpe_table,
                              void* const* page_table, int* lengths, int* decoder_result,
                              int n_batch, int n_vocab, int n_sequence, int emb_dim,
                              int n_decoder_results, int i_decoder, int elem,
                              const float* temperature, const int* top_k, const float* top_p, const int64_t* seed,
                              void* scratch, size_t scratch_bytes, void* stream);

/* EXTENSION: per-token log-probabilities and top-n alternatives from the sampled heads.  The token is the
 * one the plain entry point emits on the same inputs (bit-identical, greedy rows included); beside it the head reports,
 * for a row with logits x[0..V) whose candidates are the finite x (as in the draw),
 *   logprob(v) = (x_v - m) - log(sum over candidates of exp(x_u - m)),   m = the largest candidate.
 * These are natural-log probabilities of the RAW model distribution: they do not depend on the row's temperature, top_k,
 * top_p or seed, so greedy and sampled rows report on one scale (the common "raw logprobs" convention; the distribution
 * a sampled token was actually drawn from is the tempered, truncated one).
 *   token_logprob [n_batch * n_decoder_results]         logprob of the emitted token
 *   top_ids       [n_batch * n_decoder_results, n_top]  the n_top candidates of largest logit, ordered by (logit
 *   top_logprobs  [n_batch * n_decoder_results, n_top]  descending, index ascending), and their logprobs
 * all strided like decoder_result: row b reports at b * n_decoder_results + i_decoder (mli_sample_tokens_logprobs: at b).
 * n_top in 0 .. MLI_MAX_TOP_LOGPROBS; the selection compares fp32 values and does no arithmetic.  With fewer than n_top
 * candidates the remaining entries are id -1, logprob -inf.  An emitted token that is among the alternatives has the same
 * bits in both places.  A row that emits no token (an empty row, or no finite logit: token -1) reports -inf, ids -1 and
 * logprobs -inf.  An emitted token whose own logit is -inf reports -inf, one whose logit is +inf or NaN reports NaN (the
 * greedy pick takes a +inf); nothing faults on any device value.  The figures depend on the row's logits and n_vocab only
 * (fixed summation order, expf / logf) and are run-to-run deterministic.
 * MLI_ERR_BAD_ARG, checked before anything else and before any launch: n_top < 0, n_top > MLI_MAX_TOP_LOGPROBS, a null
 * token_logprob, null top_ids / top_logprobs with n_top > 0.  Otherwise every refusal and the scratch contract
 * (mli_sample_scratch_bytes / mli_decoder_sampled_scratch_bytes) of the plain entry points.  The contiguous form takes
 * n_decoder_results / i_decoder for the three outputs and decoder_result alike. */
#define MLI_MAX_TOP_LOGPROBS 8
int mli_sample_tokens_logprobs(const float* logits, const float* temperature, const int* top_k, const float* top_p,
                               const int64_t* seed, const int* lengths, int* tokens,
                               float* token_logprob, int* top_ids, float* top_logprobs,
                               int n_batch, int n_vocab, int n_top, void* scratch, size_t scratch_bytes, void* stream);
int mli_decoder_sampled_logprobs(const float* batch_result, const float* emb_table, const float* wpe_table,
                                 float* inp_embedding, int* lengths, int* decoder_result,
                                 int n_batch, int n_vocab, int n_sequence, int emb_dim,
                                 int n_decoder_results, int i_decoder,
                                 const float* temperature, const int* top_k, const float* top_p, const int64_t* seed,
                                 float* token_logprob, int* top_ids, float* top_logprobs, int n_top,
                                 void* scratch, size_t scratch_bytes, void* stream);
int mli_paged_decoder_sampled_logprobs(const float* batch_result, const float* emb_table, const float* wpe_table,
                                       void* const* page_table, int* lengths, int* decoder_result,
                                       int n_batch, int n_vocab, int n_sequence, int emb_dim,
                                       int n_decoder_results, int i_decoder, int elem,
                                       const float* temperature, const int* top_k, const float* top_p, const int64_t* seed,
                                       float* token_logprob, int* top_ids, float* top_logprobs, int n_top,
                                       void* scratch, size_t scratch_bytes, void* stream);

/* EXTENSION: PROMPT log-probabilities.  The decode path computes attention and logits for a row's last
 * position only; these entry points compute them for the positions of a prompt, from the pages a prefill has written.
 * SEGMENTS name the positions: segment i is (seg_row[i], seg_first[i], seg_count[i], seg_offset[i]) -- its query j is position
 * t = seg_first + j of batch row seg_row, 0 <= t < n_sequence, and lives in row seg_offset + j of the dense arrays (q, out,
 * token_logprob, top_*: n_q or n_positions rows).  The four arrays are device arrays of n_seg ints; n_seg and max_count (>= every
 * seg_count, <= n_sequence) are host integers, so every grid is known without a read-back.  A row may have several segments (a
 * prompt longer than one pass continues with seg_first > 0), segments may come in any order; two segments that share an offset
 * race.  A segment that does not lie inside (n_batch, n_sequence, the dense arrays) is skipped whole, a null page reads as
 * zeros or gathers nothing: nothing faults on any device value.  A dense row that belongs to no query is never written.
 *
 * mli_prompt_scan_paged -- the causal multi-query paged scan: query t attends slot s of its row iff s <= t and (no window, or
 *   s > t - window, or s < n_sink), one softmax per head over q_h . K_h / sqrtf(head_dim), query head h on K/V head
 *   h / (n_heads / n_kv_heads): what mli_decode_scan_paged[_heads / _window / _sinks / _gqa] compute for a row of length t + 1
 *   (fp32 rounding apart).  window <= 0 or >= n_sequence: none; n_sink without a window, or n_sink + window >= n_sequence: none.
 *   One launch ("scan_prompt"), no workspace: a workgroup streams the pages a block of mli_prompt_scan_tq consecutive queries
 *   attends once and shares every K / V load among them; no byte of a slot a query does not attend is multiplied, and the
 *   table entries of the pages between the sinks and a block's window are never read.  Shapes: fp32 / bf16 pages with rows of
 *   at most two 16-byte lane loads -- one head: MLI_ELEM_F32 to emb_dim 512, MLI_ELEM_BF16 to 1024; several heads and grouped
 *   K/V heads: what mli_decode_scan_paged_heads / _gqa take; n_batch <= 16384.  MLI_ERR_BAD_ARG before any launch: every
 *   other shape, MLI_ELEM_FP8, n_seg < 0, window < 0, n_sink < 0, and with n_seg > 0 a null pointer, max_count outside
 *   1 .. n_sequence or n_q < 1.  n_seg == 0 is a no-op returning 0.
 * mli_prompt_scan_tq -- the queries per workgroup of the variant (emb_dim, n_heads > 1, elem) runs: 8, 4 or 2 (tests place
 *   their segment edges by it); MLI_ERR_BAD_ARG for a row the scan does not take.
 * mli_prompt_project_q -- q[i] = x(row, pos) . Wq for every position of the segments: x from segment 0 of the pages, gathered
 *   into `gathered` (n_q * emb_dim page elements, 16-byte aligned) and multiplied by one MFMA GEMM launch; fp32 x and Wq on
 *   fp32 pages, bf16 x and Wq with fp32 accumulation on bf16 pages, q fp32: the decode projection's weights and rounding.
 *   The one exception to "never written": the product covers all n_q rows, so a q row that belongs to no position (a hole
 *   between segments, a tail, a skipped segment) is written too -- with the product of whatever `gathered` held in that row --
 *   and `gathered` itself is scratch.  The scan reads the q rows of its queries only.  At most 65535 segments.
 * mli_score_tokens_logprobs -- the figures of mli_sample_tokens_logprobs (raw distribution, finite candidates, the same
 *   summation order, n_top <= MLI_MAX_TOP_LOGPROBS alternatives ordered by (logit, index)) for the token targets[i] it is
 *   GIVEN.  A target outside [0, n_vocab) reports -inf for the token and the alternatives all the same.  Where the target is
 *   the token mli_sample_tokens_logprobs emits, token_logprob has the same bits.  n == 0 is a no-op; the refusals are that
 *   entry point's.
 * mli_paged_prompt_logprobs -- projection, scan, logits (attention . emb_table^T) and scoring for one list of segments; the
 *   target of position t of row b is inp[b, t + 1] (inp [n_batch, n_sequence] token ids; -1, hence -inf, at the last position).
 *   The segments' offsets tile [0, n_positions).  scratch: mli_prompt_logprobs_scratch_bytes (0 for a non-positive argument);
 *   null or too small is MLI_ERR_WORKSPACE, no byte beyond that size is written.  Refusals: the scan's and the scoring's. */
int mli_prompt_scan_tq(int emb_dim, int n_heads, int elem);
int mli_prompt_scan_paged(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                          const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                          int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int window, int n_sink, int elem,
                          void* stream);
int mli_prompt_project_q(const void* const* page_table, const int* seg_row, const int* seg_first, const int* seg_count,
                         const int* seg_offset, const void* wq, void* gathered, float* q, int n_seg, int max_count, int n_q,
                         int n_batch, int n_sequence, int emb_dim, int elem, void* stream);
int mli_score_tokens_logprobs(const float* logits, const int* targets, float* token_logprob, int* top_ids,
                              float* top_logprobs, int n, int n_vocab, int n_top, void* stream);
size_t mli_prompt_logprobs_scratch_bytes(int n_positions, int emb_dim, int n_vocab);
int mli_paged_prompt_logprobs(const void* const* page_table, const int* inp, const void* wq, const float* emb_table,
                              const int* seg_row, const int* seg_first, const int* seg_count, const int* seg_offset,
                              float* token_logprob, int* top_ids, float* top_logprobs, int n_seg, int max_count,
                              int n_positions, int n_batch, int n_sequence, int emb_dim, int n_vocab, int n_heads,
                              int n_kv_heads, int window, int n_sink, int elem, int n_top, void* scratch, size_t scratch_bytes,
                              void* stream);

/* EXTENSION: the two calls above with logit soft-capping (mli_decode_scan_paged_softcap has the formula): query t of a segment
 * gets what the capped decode scan gives a row of length t + 1, so a prompt is scored under the model that decodes.  One launch
 * ("scan_prompt_softcap") with the SAME queries per workgroup as the uncapped variant: mli_prompt_scan_tq holds for both (the
 * capped kernels compile without scratch at it).  Scratch: mli_prompt_logprobs_scratch_bytes.  MLI_ERR_BAD_ARG before any
 * launch: n_heads == 1, cap <= 0, NaN or infinite, and everything the uncapped call refuses (fp8 pages among it). */
int mli_prompt_scan_paged_softcap(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                  const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                                  int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int window, int n_sink,
                                  float cap, int elem, void* stream);
int mli_paged_prompt_logprobs_softcap(const void* const* page_table, const int* inp, const void* wq, const float* emb_table,
                                      const int* seg_row, const int* seg_first, const int* seg_count, const int* seg_offset,
                                      float* token_logprob, int* top_ids, float* top_logprobs, int n_seg, int max_count,
                                      int n_positions, int n_batch, int n_sequence, int emb_dim, int n_vocab, int n_heads,
                                      int n_kv_heads, int window, int n_sink, float cap, int elem, int n_top, void* scratch,
                                      size_t scratch_bytes, void* stream);

/* EXTENSION: mli_prompt_scan_paged and mli_paged_prompt_logprobs with learned sink logits (mli_decode_scan_paged_sink_logits has
 * the formula): query t of a segment gets what the decode scan with the same logits gives a row of length t + 1, so a prompt is
 * scored under the model that decodes.  One launch ("scan_prompt_sink_logits") with the SAME queries per workgroup as the plain
 * variant: mli_prompt_scan_tq holds.  All logits -inf give the plain call's bits.  Scratch: mli_prompt_logprobs_scratch_bytes.
 * MLI_ERR_BAD_ARG before any launch: n_heads == 1, a null sink_logits, and everything the plain call refuses (fp8 pages among
 * it). */
int mli_prompt_scan_paged_sink_logits(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                      const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                                      int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int window,
                                      int n_sink, const float* sink_logits, int elem, void* stream);
int mli_paged_prompt_logprobs_sink_logits(const void* const* page_table, const int* inp, const void* wq, const float* emb_table,
                                          const int* seg_row, const int* seg_first, const int* seg_count, const int* seg_offset,
                                          float* token_logprob, int* top_ids, float* top_logprobs, int n_seg, int max_count,
                                          int n_positions, int n_batch, int n_sequence, int emb_dim, int n_vocab, int n_heads,
                                          int n_kv_heads, int window, int n_sink, const float* sink_logits, int elem, int n_top,
                                          void* scratch, size_t scratch_bytes, void* stream);

/* PREFILL of the newly inserted rows in ONE launch: the encoder as the fill GEMM's prologue.  The A
 * tile rows are computed on the fly as emb_table[inp[b, s]] + wpe[s] -- nothing is read back from the input-embedding
 * segment -- multiplied by [Wk | Wv], and the workgroups of the first column tile also write those rows to segment 0
 * (the decode projection reads position L - 1 from there).  Pages / caches come out bit-identical to
 *   mli_paged_attention_encoder[_bf16] + mli_fill_new_k_v_cache_paged[_bf16]   (paged; elem_bf16 selects the element type)
 *   mli_inference_optimized_encoder + mli_fill_new_kt_v_cache                   (contiguous)
 * i.e. launch_paged_attention_encoder_kernel + launch_fill_new_k_v_cache_paged_attention[_warp_tiling]
 * (encoder.h:22-25, paged_attention.h:28-30,65-67) resp. launch_inference_optimized_encoder_kernel +
 * launch_fill_new_kt_v_cache (encoder.h:16-19, self_attention_inference_optimized.h:5-8).  No-op when n_new_items == 0.
 * Since round 3 the entry points pick the form by shape (mli_tune "prefill_fused"): the prologue form up to emb_dim 512, those
 * two launches beyond -- every column tile of the prologue form re-reads the fp32 embedding and position rows, which wide
 * models (many column tiles) pay more for than for one launch boundary (emb_dim 2048: 199 us against 154 + 14 us). */
int mli_paged_prefill(const float* emb_table, const float* wpe, const int* inp, void* const* page_table,
                      const int* lengths, const int* new_item_indices, const void* wk, const void* wv,
                      int n_batch, int n_sequence, int emb_dim, int n_new_items, int elem_bf16, void* stream);
int mli_prefill(const float* emb_table, const float* wpe, const int* inp, float* inp_embedding, const int* lengths,
                const int* new_item_indices, const float* wk, const float* wv, float* kt_cache, float* v_cache,
                int n_batch, int n_sequence, int input_dim, int output_dim, int n_new_items, void* stream);
/* EXTENSION: mli_paged_prefill of the LIVE tokens of rows that decode under a sliding window with attention sinks (the
 * scans of mli_paged_attention_lean_window / _sinks).  For a row of L tokens, p0 = max(0, L - window) / 16 and ps =
 * ceil(n_sink / 16): pages ps <= i < p0 are dead -- no decode step of the row reads them, now or at any later length.
 *   live pages receive the bits mli_paged_prefill writes to them (x, K and V segments), in the same form (prologue form, or
 *     encoder + fill, by mli_tune "prefill_fused");
 *   the table entry of a dead page is never read and no byte of the page is written: it may be null, stale, or name a page
 *     of another row.  No GEMM tile is spent on a dead token: the cost follows min(L, n_sink + window).
 * window == 0 (none), window >= n_sequence and n_sink + window >= n_sequence leave no row a dead page and ARE
 * mli_paged_prefill; window < 0 or n_sink < 0 is MLI_ERR_BAD_ARG.  Shapes and element types are mli_paged_prefill's. */
int mli_paged_prefill_window(const float* emb_table, const float* wpe, const int* inp, void* const* page_table,
                             const int* lengths, const int* new_item_indices, const void* wk, const void* wv,
                             int n_batch, int n_sequence, int emb_dim, int n_new_items, int window, int n_sink, int elem,
                             void* stream);

/* One whole decode step of the continuous batch (n_new_items = 0) in ONE call: what *InferenceModel::forward does per
 * round once the new rows are prefilled (reference src/inference_model.cpp:26-30, 68-72) -- lean attention
 * (mli_paged_attention_lean / mli_self_attention_lean) followed by the fused decoder head.  For hosts that pay per
 * call (the Python test / bench front end); the C++ layers issue the same launches themselves.
 *   paged:      q_output [n_batch, emb_dim] is scratch; attention_result [n_batch, emb_dim] holds the attention output
 *   contiguous: qkt_output [n_batch, n_sequence] is scratch for the shapes mli_self_attention_lean does not cover
 * The workspace must have been initialised once (mli_attention_workspace_init). */
int mli_paged_decode_step(void* const* page_table, int* lengths, const void* wk, const void* wq, const void* wv,
                          const float* emb_table, const float* wpe_table, float* q_output, float* attention_result,
                          int* decoder_result, int n_batch, int n_sequence, int emb_dim, int n_vocab,
                          int n_decoder_results, int i_decoder, int elem_bf16,
                          void* workspace, size_t workspace_bytes, void* decoder_scratch, size_t decoder_scratch_bytes,
                          void* stream);
int mli_decode_step(float* inp_embedding, int* lengths, const float* wk, const float* wq, const float* wv,
                    const float* emb_table, const float* wpe_table, float* kt_cache, float* v_cache,
                    float* q_output, float* qkt_output, float* attention_result, int* decoder_result,
                    int n_batch, int n_sequence, int emb_dim, int n_vocab,
                    void* workspace, size_t workspace_bytes, void* decoder_scratch, size_t decoder_scratch_bytes,
                    void* stream);

/* ------------------------------------------------------------------------------------
 * hipGraph capture of a decode step.  No entry point above allocates or synchronises, so any sequence of them issued
 * on one (non-default) stream between begin and end becomes a graph; replaying it costs one host call instead of one
 * per kernel.  A decode step with n_new_items == 0 is replay-safe: its launches depend on device state (lengths,
 * page table, pages) only through pointers, never through host-side values.  What the engines' forward() replays
 * (reference loop: src/inference_model.cpp:56-81).
 * ---------------------------------------------------------------------------------- */
int mli_graph_begin_capture(void* stream);                      /* stream must not be the legacy default stream */
int mli_graph_end_capture(void* stream, void** graph_exec_out); /* ends the capture and instantiates it */
int mli_graph_launch(void* graph_exec, void* stream);
/* `waiter` does not run anything queued after this call before everything queued on `signaller` so far has run (an
 * event recorded on one stream and waited for on the other).  Inside a capture it adds a dependency edge -- and pulls
 * `waiter` into the capture --, which is how a captured step forks into parallel branches (e.g. two micro-batches of
 * the batch rows: one half's memory-bound scan beside the other half's latency-bound GEMMs) and joins again. */
int mli_stream_wait_stream(void* waiter, void* signaller);
int mli_graph_destroy(void* graph_exec);

/* ------------------------------------------------------------------------------------
 * Test / measurement support (not on the reference's product path).
 * ---------------------------------------------------------------------------------- */

/* replaces launch_clone_inp_embedding_k_v_cache (include/utils.h:101-103, src/kernels/utils.cu:230-239):
 * copies contiguous inp/kt/v tensors into the pages of every non-empty row, positions
 * 0..min(length, n_sequence-1) inclusive. */
int mli_clone_inp_embedding_k_v_cache(float* const* page_table, const float* inp_embedding,
                                      const float* kt_cache, const float* v_cache, const int* lengths,
                                      int n_batch, int n_sequence, int emb_dim, void* stream);

/* fp32 -> fp8 (OCP e4m3fn; round to nearest even, saturating at +-448, NaN kept) with the conversion the fp8 page kernels
 * use: n (a multiple of 4) values.  For building synthetic fp8 pages in tests and bench.py. */
int mli_f32_to_fp8(const float* src, uint8_t* dst, size_t n, void* stream);

/* Tuning / diagnostic knobs.  PER THREAD: a setting applies to the launches the calling thread issues afterwards, so a test
 * or a probe never changes what an engine on another thread runs (results are identical for every setting):
 *   "chunk_tokens"     0 = heuristic, else a power of two in [64, 1024]: tokens per workgroup of the
 *                      split-sequence kernels
 *   "nt_loads"         non-temporal hint on the K/V stream: 2 (default) = where the rows' K/V (n_batch * n_sequence *
 *                      emb_dim * 2 elements) exceeds 768 MiB, i.e. nothing of it survives in the 256 MiB Infinity Cache
 *                      until the next step; 1 = always, 0 = never (plain loads)
 *   "scan_resident_mib"  (equal page shares, where the K/V stream is non-temporal) MiB of the launch's K/V, 0 .. 240 (default
 *                      192), that are loaded with the default policy instead: a slice of the pages chosen by address, the
 *                      same in every step, which the non-temporal loads of the rest leave in the Infinity Cache, so a
 *                      decode step finds it on die.  0 = every load non-temporal.  Identical results for every value.
 *                      (Rows wider than 64 16-byte lane loads keep their loads non-temporal and touch the lines of a
 *                      kept page with default-policy loads first.)
 *   "scan_stream"      (lean mode) 1 (default) = batches that fill the chip (n_batch * n_sequence >= 2^21, n_batch <= 2048,
 *                      n_sequence >= 1024) are scanned in EQUAL PAGE SHARES: the pages of all rows form one sequence
 *                      that 2 x CUs workgroups split evenly, each streaming its share across row boundaries and merging
 *                      per row like "scan_merge" (attention_stream.hip); 0 = always one workgroup per (row, chunk).
 *                      Same result for the same lengths on every launch; against the chunked form the split points of
 *                      a row differ, i.e. the fp32 rounding of the merge (<= 1e-5 on attention_result).
 *                      The chunked scan runs instead, silently and with the same contract ("scan_chunked" counts, not
 *                      "scan_equal_shares"), wherever one of these holds: n_batch > 2048; n_sequence < 1024; n_batch *
 *                      n_sequence below "scan_stream_min_tokens"; rows of more than two 16-byte lane loads; a row's
 *                      n_sequence / 64 statistics pairs larger than the kernel's q buffer (8 * ceil(n_sequence / 64) >
 *                      MAXSEG * emb_dim * 4 with MAXSEG = 4, or 2 for bf16 / fp8 rows of 1024 columns: fp32 emb_dim 64
 *                      stops at n_sequence 8192); or more than 80 KiB of LDS per workgroup, which grows with n_batch and
 *                      with n_batch * n_sequence / CUs (2048 rows of emb_dim 512 on 256 CUs: n_sequence 14336 is taken
 *                      with 76.25 KiB, 16384 would need 80.25 KiB).  From 64 KiB on the launcher raises the kernel's
 *                      dynamic-LDS limit first.
 *   "scan_stream_min_tokens"  the n_batch * n_sequence threshold of "scan_stream" (tests lower it)
 *   "scan_stream_dynamic_pct" / "scan_stream_granule"  the last x per cent (default 4, at most 12; 0 = none) of the page
 *                      sequence are not part of the equal shares but handed out by a ticket counter in granules of that
 *                      many pages (default 64, 16..256) to the workgroups that finish their share first
 *   "scan_merge"       (lean mode) 1 (default) = the workgroup that completes a row merges its chunks inside the scan
 *                      launch, 0 = a separate combine launch; bit-identical results
 *   "fused_softmax"    (separate-pass form only) 1 = the compositions fold the masked softmax into the qkt / softmax.V kernels, 0 = three
 *                      launches as the reference (qkt, softmax_in_place_with_lengths, softmax_v), -1 (default) =
 *                      fuse when n_batch * n_sequence <= 2^20 (launch-bound steps)
 *   "fill_compact"     1 (default) = the prefill GEMM runs over the flat list of (new row, token) pairs, 0 = one tile
 *                      grid per new row (the reference's decomposition); bit-identical results
 *   "latest_compact"   1 (default) = the decode projection multiplies a device-built list of the non-empty batch rows where
 *                      the reduction is >= 1024 long (building the list costs every workgroup ~2 us), 2 = wherever
 *                      possible, 0 = all rows (empty ones as zeros); identical results
 *   "scan_row_order"   1 (default) = single-pass scans with one workgroup per row (short sequences) and more than 512 rows
 *                      hand the rows out longest first, 0 = in grid order (identical results)
 *   "gemm_split"       1 (default) = the fp32 GEMM with 64-row tiles (prefill, logits, projections of batches that do not
 *                      fill the chip with 128-row tiles) runs as 512-thread workgroups, four waves loading and four
 *                      multiplying, when the reduction is >= 256 long; 0 = one wave does both (identical results)
 *   "gemm_bf16_split"  1 (default) = the bf16 decode projection at emb_dim >= 1536 (any batch) or >= 1024 (from 320 rows),
 *                      emb_dim a multiple of 64, runs the loader-wave / MFMA-wave kernel (LDS-DMA loaders, 128 x 192 tiles, one
 *                      per CU at 1024 rows), 0 = the tiled kernels (identical results)
 *   "prefill_fused"    1 (default) = mli_[paged_]prefill runs the encoder as the fill GEMM's prologue up to emb_dim 512 and
 *                      encoder + fill as two launches beyond, 0 = always two launches, 2 = always the prologue form (fp8 pages
 *                      have the prologue form only); pages / caches are bit-identical either way
 *   "gemm_panel"       1 (default) = small fp32 products (emb_dim <= 512, fewer than 256 tiles of 64x64: the decode
 *                      projection and the logits of configs 2 / 3) run the latency-shaped kernel (32x32 tiles, the
 *                      whole K panel requested at once), 0 = always the tiled kernel, 2 = whenever the shape allows
 *                      (lets tests push other shapes through it); bit-identical results
 *   "gemm_tall_tiles"  1 (default) = 128x64 workgroup tiles for the decode projection / logits GEMM (fp32 and bf16)
 *                      when the grid still fills the chip, 0 = always 64x64, 2 = 128x64 whenever the mode allows it
 *                      (lets small test shapes exercise that kernel)
 *   "bf16_native_mfma" 1 (default) = v_mfma_f32_32x32x16_bf16 tile engine for the bf16 path, 0 = operands widened
 *                      to fp32 + fp32 MFMA (bit-identical to a sequential fp32 sum; differs from 1 only by the
 *                      rounding order of the fp32 accumulation) */
int mli_tune(const char* key, int value);

/* Launch counters: which branch of a launcher the calling thread's calls took.  PER THREAD, like the knobs above: an engine
 * runs in its caller's thread, so the caller reads what its own engine launched, and nothing another thread runs is seen.
 * Host side only: a counter is incremented where the launcher enqueues the kernel (one increment per launch); no kernel reads
 * or writes them and no kernel differs for them.  A launch enqueued while its stream is being captured into a graph counts
 * ONCE, at capture; replays of the graph do not count.  A launcher that answers "not applicable" or refuses its arguments
 * before enqueueing counts nothing -- a silent hand-back to another kernel shows as that kernel's count.
 * mli_launch_count stores the count of `family` since the thread's last reset (0 at thread start) in *count; MLI_ERR_BAD_ARG
 * for a null or unknown name or a null count, which is left untouched.  mli_launch_counts_reset zeroes every family.
 * Kernel families (a launch of one of these kernels counts in exactly one; other kernels are not counted):
 *   "gemm_f32_panel"         fp32 GEMM, latency-shaped 32x32 kernel ("gemm_panel")
 *   "gemm_f32_rows64"        fp32 GEMM, 64-row tiles, one wave loads and multiplies
 *   "gemm_f32_rows64_split"  fp32 GEMM, 64-row tiles, loader waves + MFMA waves ("gemm_split")
 *   "gemm_f32_rows128"       fp32 GEMM, 128-row tiles ("gemm_tall_tiles")
 *   "gemm_bf16_widened"      bf16 pages through the fp32 MFMA kernel ("bf16_native_mfma" 0), projection and fill
 *   "gemm_bf16_rows64"       bf16 / fp8 decode projection, 64-row tiles, 32 k per stage
 *   "gemm_bf16_deep"         ... 64-row tiles, 128 k per stage (emb_dim 256 .. 1024)
 *   "gemm_bf16_rows128"      ... 128-row tiles ("gemm_tall_tiles")
 *   "gemm_bf16_dma"          ... the LDS-DMA loader-wave / MFMA-wave kernel ("gemm_bf16_split")
 *   "gemm_bf16_fill"         the prefill fill of bf16 / fp8 pages (native MFMA)
 *   "scan_equal_shares"      the equal-page-shares scan ("scan_stream")
 *   "scan_chunked"           the single-head chunked scan, lean or materialising, every grid form
 *   "scan_heads_window"      the scans with several heads, a window, sinks or grouped K/V heads
 *   "scan_prompt"            the causal multi-query scan over prompt positions (mli_prompt_scan_paged)
 *   "scan_heads_alibi"       the multi-head scans with a position bias per head (mli_decode_scan_paged_alibi)
 *   "scan_heads_softcap"     the multi-head scans with logit soft-capping (mli_decode_scan_paged_softcap)
 *   "scan_prompt_softcap"    the prompt scan with logit soft-capping (mli_prompt_scan_paged_softcap)
 *   "scan_heads_sink_logits" the multi-head scans with a learned sink logit per query head (mli_decode_scan_paged_sink_logits)
 *   "scan_prompt_sink_logits" the prompt scan with a learned sink logit per query head (mli_prompt_scan_paged_sink_logits)
 * Forms, counted beside the launch's kernel family:
 *   "latest_compact"         a decode projection over the compacted list of non-empty rows ("latest_compact"; the panel and
 *                            the LDS-DMA kernel have no such list)
 *   "gemm_f32_rope" / "gemm_bf16_rope"   a tiled fp32-MFMA / bf16-MFMA form with rotary position embeddings (the *_rope entry
 *                            points; also at the shapes that would take "gemm_f32_panel" / "gemm_bf16_dma" without a table)
 *   "fill_flat" / "fill_per_row"   a prefill fill over the flat (new row, token) list / one tile grid per new row ("fill_compact")
 *   "prefill_fused" / "prefill_two_launch"   mli_prefill, mli_paged_prefill[_window] with new rows: the encoder as the fill's
 *                            prologue / encoder + fill ("prefill_fused")
 *   "scan_rows_ordered" / "scan_rows_grid_order"   a "scan_chunked" launch with one workgroup per row: rows handed out longest
 *                            first / in grid order ("scan_row_order") */
int mli_launch_count(const char* family, unsigned long long* count);
int mli_launch_counts_reset(void);

/* The resident slice of "scan_resident_mib", restated for tests and tools.  mli_scan_resident_threshold: the threshold
 * (0 .. 65536) of a launch whose rows hold total_pages pages in all (elem: MLI_ELEM_*; MLI_ERR_BAD_ARG for another tag, a
 * negative page count or emb_dim <= 0).  mli_scan_resident_keeps: 1 if that launch loads the page at page_ptr with the
 * default policy, 0 if non-temporal; a function of the address and the threshold only, monotone in the threshold. */
int mli_scan_resident_threshold(long long total_pages, int emb_dim, int elem, int resident_mib);
int mli_scan_resident_keeps(const void* page_ptr, int thr);

/* float4 device copy (kept for tools; a copy is not a ceiling for a read stream). */
int mli_stream_copy(const float* src, float* dst, size_t n_floats, void* stream);
/* Pure streaming read of n_floats (a multiple of 16384) with the scan's load shape -- 16-byte non-temporal lane loads,
 * 16 KiB per wave in flight, nothing written: the box's read-only HBM rate, which bench.py reports beside the scan's
 * (`roofline.measured_read_gbs`).  sink: >= 1 float of device memory, never written in practice. */
int mli_stream_read(const float* src, float* sink, size_t n_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MLI_KERNELS_H */
