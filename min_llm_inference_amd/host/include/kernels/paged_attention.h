// Paged-KV decode attention launchers with the reference's signatures
// (include/kernels/paged_attention.h:17-67).  page_table is [n_batch, n_sequence / PAGE_BLOCK_SIZE] device
// pointers to blocks of PAGE_BLOCK_SIZE * 3 * emb_dim floats (input embedding | K | V per token).
#pragma once

#include "tensor.hpp"

// The reference threads a cublasHandle_t through its cuBLAS variants.  The MFMA kernels need no library
// handle; GemmHandle is an empty tag that keeps the parameter position, so a call site changes one type name.
struct GemmHandle {};

void paged_attention(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorFloat& wk,
                     const TensorFloat& wq, const TensorFloat& wv, const TensorInt& new_batch_idx,
                     TensorFloat& q_output, TensorFloat& qkt_output, TensorFloat& attention_result, int n_new_items,
                     int n_sequence);

void launch_fill_new_k_v_cache_paged_attention(TensorFloatPoint page_table, const TensorInt& new_batch_idx,
                                               const TensorInt& lengths, const TensorFloat& wk,
                                               const TensorFloat& wv, int n_new_items, int n_sequence);

void launch_get_latest_k_q_v_paged_attention(TensorFloatPoint& page_table, const TensorInt& lengths,
                                             const TensorFloat& wk, const TensorFloat& wq, const TensorFloat& wv,
                                             TensorFloat& q_output, int n_sequence);

void launch_qkt_paged_attention(const TensorFloat& q_output, const TensorFloatPoint& page_table,
                                const TensorInt& lengths, TensorFloat& qkt_output);

void launch_softmax_v_paged_attention(const TensorFloat& softmax_result, const TensorFloatPoint& page_table,
                                      TensorFloat& attention_result, const TensorInt& lengths);

// EXTENSION (no reference counterpart): paged_attention without materialising scores / probabilities -- q_output and
// attention_result come out bit-identical, qkt_output is left alone (it is only used when emb_dim exceeds what the
// single-pass kernel covers).  What PagedAttention[Cublas]Layer::forward runs unless runtime::set_lean_layers(false).
void paged_attention_lean(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorFloat& wk,
                          const TensorFloat& wq, const TensorFloat& wv, const TensorInt& new_batch_idx,
                          TensorFloat& q_output, TensorFloat& qkt_output, TensorFloat& attention_result,
                          int n_new_items, int n_sequence);

// EXTENSION: paged_attention_lean with n_heads attention heads (head h owns columns [h * emb_dim / n_heads, ...) of q, K
// and V; one softmax per head).  Pages and q_output are those of paged_attention_lean.  Throws on an unsupported shape.
void paged_attention_lean_heads(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorFloat& wk,
                                const TensorFloat& wq, const TensorFloat& wv, const TensorInt& new_batch_idx,
                                TensorFloat& q_output, TensorFloat& attention_result, int n_new_items, int n_sequence,
                                int n_heads);

// EXTENSION: paged_attention_lean[_heads] with a sliding window: row b attends its newest `window` tokens (slots
// [max(0, L - window), L), L = min(lengths[b], n_sequence)).  Pages and q_output are those of paged_attention_lean;
// window >= n_sequence is the un-windowed call.  Throws on an unsupported shape.
void paged_attention_lean_window(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorFloat& wk,
                                 const TensorFloat& wq, const TensorFloat& wv, const TensorInt& new_batch_idx,
                                 TensorFloat& q_output, TensorFloat& attention_result, int n_new_items, int n_sequence,
                                 int n_heads, int window);

// EXTENSION: paged_attention_lean_window with attention sinks: row b attends its first n_sink tokens as well as its newest
// `window` (slots s < L with s < n_sink or s >= max(0, L - window)).  n_sink == 0 is paged_attention_lean_window; n_sink +
// window >= n_sequence is the un-windowed call.  Throws on an unsupported shape.
void paged_attention_lean_sinks(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorFloat& wk,
                                const TensorFloat& wq, const TensorFloat& wv, const TensorInt& new_batch_idx,
                                TensorFloat& q_output, TensorFloat& attention_result, int n_new_items, int n_sequence,
                                int n_heads, int window, int n_sink);

// EXTENSION: paged_attention_lean_sinks with grouped-query attention: n_kv_heads K/V heads (a divisor of n_heads) serve the
// n_heads query heads, head h attending K/V head h / (n_heads / n_kv_heads); window <= 0 or >= n_sequence = none, n_sink 0 =
// no sinks.  wk / wv keep their [emb_dim, emb_dim] shape: their first n_kv_heads * emb_dim / n_heads output columns matter.
void paged_attention_lean_gqa(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorFloat& wk,
                              const TensorFloat& wq, const TensorFloat& wv, const TensorInt& new_batch_idx,
                              TensorFloat& q_output, TensorFloat& attention_result, int n_new_items, int n_sequence, int n_heads,
                              int n_kv_heads, int window, int n_sink);

// What the five functions above share, and what the fp32 layers call: n_heads heads, window <= 0 or >= n_sequence = none,
// n_sink sinks beside a window, n_kv_heads K/V heads (0: as many as n_heads); qkt_output (may be null) serves one head without a
// window as in paged_attention_lean.
void paged_attention_lean_layer(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorFloat& wk,
                                const TensorFloat& wq, const TensorFloat& wv, const TensorInt& new_batch_idx,
                                TensorFloat& q_output, TensorFloat* qkt_output, TensorFloat& attention_result,
                                int n_new_items, int n_sequence, int n_heads, int window, int n_sink, int n_kv_heads = 0);

// EXTENSION: launch_paged_attention_encoder_kernel + launch_fill_new_k_v_cache_paged_attention in one
// launch -- the embedding lookup is the fill GEMM's prologue; pages bit-identical to the two-launch form.
void launch_paged_prefill(const TensorFloat& emb_table, const TensorFloat& wpe, const TensorInt& inp,
                          TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_item_indices,
                          const TensorFloat& wk, const TensorFloat& wv, int n_new_items);
// ... of the live tokens of rows that decode under (window, n_sink) and return their dead pages early
// (mli_paged_prefill_window; no effective window: launch_paged_prefill)
void launch_paged_prefill_window(const TensorFloat& emb_table, const TensorFloat& wpe, const TensorInt& inp,
                                 TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_item_indices,
                                 const TensorFloat& wk, const TensorFloat& wv, int n_new_items, int window, int n_sink);
// What the two above and every paged layer's prefill() run: pages of elem = MLI_ELEM_*, wk / wv that type's weights;
// live_only = launch_paged_prefill_window under (window, n_sink).  n_new_items == 0 launches nothing.
// rope_table (EXTENSION, [n_sequence][emb_dim / n_heads / 2] (cos, sin) in device memory; null: none): K is stored rotated by
// the token's slot (mli_paged_prefill_rope), live_only or not.
void launch_paged_prefill_elem(const TensorFloat& emb_table, const TensorFloat& wpe, const TensorInt& inp,
                               TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_item_indices,
                               const void* wk, const void* wv, int n_new_items, int elem, bool live_only, int window,
                               int n_sink, int n_heads = 1, const float* rope_table = nullptr);

// "cuBLAS" variants: same results, produced by the same gather-GEMM-scatter MFMA kernel.  latest_emb and
// temp_placeholder were scratch for the three cublasSgemm calls and are accepted but not used.
void paged_attention_with_cublas(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorFloat& wk,
                                 const TensorFloat& wq, const TensorFloat& wv, const TensorInt& new_batch_idx,
                                 TensorFloat& q_output, TensorFloat& qkt_output, TensorFloat& attention_result,
                                 TensorFloat& latest_emb, TensorFloat& temp_placeholder, int n_new_items,
                                 int n_sequence, GemmHandle& handle);

void launch_get_latest_k_q_v_paged_attention_cublas(TensorFloatPoint& page_table, const TensorInt& lengths,
                                                    TensorFloat& latest_emb, const TensorFloat& wk,
                                                    const TensorFloat& wq, const TensorFloat& wv,
                                                    TensorFloat& q_output, TensorFloat& temp_placeholder,
                                                    GemmHandle& handle, int n_sequence);

void launch_fill_new_k_v_cache_paged_attention_warp_tiling(TensorFloatPoint page_table,
                                                           const TensorInt& new_batch_idx, const TensorInt& lengths,
                                                           const TensorFloat& wk, const TensorFloat& wv,
                                                           int n_new_items, int n_sequence);
