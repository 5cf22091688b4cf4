// Layer objects: own the weights and the pre-allocated scratch, unpack shapes, call the launchers.
// Same constructors and forward() signatures as the reference (include/layers.h:19-156) for the layers
// on the inference path.  FeedForward (used by no model in the reference) is out of scope.
#pragma once

#include "kernels/paged_attention.h"
#include "tensor.hpp"
#include "utils.h"

#include "kernels/decoder.h"  // SlotSampling, DecoderLogprobs

class SelfAttentionLayer : public NonCopyableNonClonable {
public:
    SelfAttentionLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch, size_t input_dim,
                       size_t n_sequence);
    void forward(const TensorFloat& inp_embedding, const TensorInt& lengths, const TensorInt& new_batch_idx,
                 TensorFloat& attention_result, int n_new_items);
    // extension: encoder + K/V prefill of the new rows in one launch (the model then calls forward with n_new_items = 0)
    void prefill(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                 TensorFloat& inp_embedding, const TensorInt& lengths, const TensorInt& new_item_indices, int n_new_items);

private:
    TensorFloat wk_, wq_, wv_;
    TensorFloat kt_cache_;    // [n_batch, input_dim, n_sequence]
    TensorFloat v_cache_;     // [n_batch, n_sequence, input_dim]
    TensorFloat q_output_;    // [n_batch, input_dim]
    TensorFloat qkt_output_;  // [n_batch, n_sequence]
};

class PagedAttentionLayer : public NonCopyableNonClonable {
public:
    PagedAttentionLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch, size_t emb_dim,
                        size_t n_sequence);
    void forward(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_batch_idx,
                 TensorFloat& attention_result, int n_new_items);
    // extension: encoder + K/V prefill of the new rows in one launch (the model then calls forward with n_new_items = 0)
    void prefill(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                 TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_item_indices,
                 int n_new_items);

    // EXTENSION: attention heads of the lean forward (default 1 = the reference's single softmax over emb_dim)
    void set_n_heads(int n_heads) { n_heads_ = n_heads; }
    // EXTENSION: grouped-query attention of the lean forward: K/V heads serving the n_heads query heads (0 = as many)
    void set_n_kv_heads(int n_kv_heads) { n_kv_heads_ = n_kv_heads; }
    // EXTENSION: sliding window of the lean forward: a row attends its newest `window` tokens (0 or >= n_sequence: all)
    void set_window(int window) { window_ = window; }
    // EXTENSION: attention sinks of the lean forward: beside a window a row keeps its first n_sink tokens attended (0: none)
    void set_sinks(int n_sink) { n_sink_ = n_sink; }
    // EXTENSION: the rows' pages below the window are returned early (PagedAttentionsManager::set_page_release): prefill
    // covers a row's live tokens only and follows no table entry of a dead page (mli_paged_prefill_window)
    void set_page_release(bool enabled) { page_release_ = enabled; }

private:
    TensorFloat wk_, wq_, wv_;
    TensorFloat q_output_;
    TensorFloat qkt_output_;
    int n_heads_ = 1;
    int n_kv_heads_ = 0;
    int window_ = 0;
    int n_sink_ = 0;
    bool page_release_ = false;
};

class PagedAttentionCublasLayer : public NonCopyableNonClonable {
public:
    PagedAttentionCublasLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch, size_t emb_dim,
                              size_t n_sequence);
    void forward(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_batch_idx,
                 TensorFloat& attention_result, int n_new_items, GemmHandle& handle);
    void prefill(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                 TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_item_indices,
                 int n_new_items);  // extension, as PagedAttentionLayer::prefill

    // EXTENSION: attention heads of the lean forward (default 1 = the reference's single softmax over emb_dim)
    void set_n_heads(int n_heads) { n_heads_ = n_heads; }
    // EXTENSION: grouped-query attention of the lean forward: K/V heads serving the n_heads query heads (0 = as many)
    void set_n_kv_heads(int n_kv_heads) { n_kv_heads_ = n_kv_heads; }
    // EXTENSION: sliding window of the lean forward: a row attends its newest `window` tokens (0 or >= n_sequence: all)
    void set_window(int window) { window_ = window; }
    // EXTENSION: attention sinks of the lean forward: beside a window a row keeps its first n_sink tokens attended (0: none)
    void set_sinks(int n_sink) { n_sink_ = n_sink; }
    // EXTENSION: the rows' pages below the window are returned early (PagedAttentionsManager::set_page_release): prefill
    // covers a row's live tokens only and follows no table entry of a dead page (mli_paged_prefill_window)
    void set_page_release(bool enabled) { page_release_ = enabled; }

private:
    TensorFloat wk_, wq_, wv_;
    TensorFloat q_output_;
    TensorFloat qkt_output_;
    int n_heads_ = 1;
    int n_kv_heads_ = 0;
    int window_ = 0;
    int n_sink_ = 0;
    bool page_release_ = false;
    TensorFloat latest_emb_;        // kept for signature parity with the reference; unused by the MFMA path
    TensorFloat temp_placeholder_;
};

// emb_table [n_vocab, dim], pos_emb [n_sequence, dim], inp [n_batch, n_sequence] token ids
class EncoderLayer : public NonCopyableNonClonable {
public:
    void forward(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                 TensorFloat& inp_embedding, const TensorInt& lengths, const TensorInt& new_item_indices,
                 int n_new_items);
};

class PagedEncoderLayer : public NonCopyableNonClonable {
public:
    void forward(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                 TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_item_indices,
                 int n_new_items);
};

class DecoderLayer : public NonCopyableNonClonable {
public:
    DecoderLayer(size_t n_batch, size_t n_vocab);
    void forward(const TensorFloat& batch_result, const TensorFloat& emb_table, const TensorFloat& wpe_table,
                 TensorFloat& inp_embedding, TensorInt& lengths, TensorInt& decoder_result);

    // EXTENSION: from now on forward() runs the sampled head with these per-slot parameters (nullptr: the greedy head)
    void set_sampling(const SlotSampling* sampling) { sampling_ = sampling; }
    // EXTENSION: the sampled head also reports log-probabilities into buffers this layer owns from now on:
    // [n_batch, n_rounds(, n_top)], n_top in 0 .. 8.  Takes effect where the sampled head runs (set_sampling).
    void set_logprobs(int n_rounds, int n_top) { logprobs_.allocate(emb_score_.shape()[0], (size_t)n_rounds, n_top); }
    const DecoderLogprobs& logprobs() const { return logprobs_; }

private:
    TensorFloat emb_score_;  // [n_batch, n_vocab]
    const SlotSampling* sampling_ = nullptr;
    DecoderLogprobs logprobs_;
};

class PagedDecoderLayer : public NonCopyableNonClonable {
public:
    PagedDecoderLayer(size_t n_batch, size_t n_vocab);
    void forward(const TensorFloat& batch_result, const TensorFloat& emb_table, const TensorFloat& wpe_table,
                 TensorFloatPoint& page_table, TensorInt& lengths, TensorInt& decoder_result, int i_decoder_round);

    void set_sampling(const SlotSampling* sampling) { sampling_ = sampling; }  // EXTENSION, as DecoderLayer's
    void set_logprobs(int n_rounds, int n_top) { logprobs_.allocate(emb_score_.shape()[0], (size_t)n_rounds, n_top); }
    const DecoderLogprobs& logprobs() const { return logprobs_; }

private:
    TensorFloat emb_score_;
    const SlotSampling* sampling_ = nullptr;
    DecoderLogprobs logprobs_;
};

class PagedCublasDecoderLayer : public NonCopyableNonClonable {
public:
    PagedCublasDecoderLayer(size_t n_batch, size_t n_vocab);
    void forward(const TensorFloat& batch_result, const TensorFloat& emb_table, const TensorFloat& wpe_table,
                 TensorFloatPoint& page_table, TensorInt& lengths, TensorInt& decoder_result, int i_decoder_round,
                 GemmHandle& handle);

    void set_sampling(const SlotSampling* sampling) { sampling_ = sampling; }  // EXTENSION, as DecoderLayer's
    void set_logprobs(int n_rounds, int n_top) { logprobs_.allocate(emb_score_.shape()[0], (size_t)n_rounds, n_top); }
    const DecoderLogprobs& logprobs() const { return logprobs_; }

private:
    TensorFloat emb_score_;
    const SlotSampling* sampling_ = nullptr;
    DecoderLogprobs logprobs_;
};
