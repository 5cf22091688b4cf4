// encoder -> attention -> decoder, once per engine iteration (reference include/inference_model.h:8-74).
#pragma once

#include "layers.h"
#include "step_graph.h"
#include "tensor.hpp"
#include "utils.h"

class InferenceModel : public NonCopyableNonClonable {
public:
    InferenceModel(SelfAttentionLayer&&, EncoderLayer&&, DecoderLayer&&, size_t n_batch, size_t n_sequence,
                   size_t emb_dim);

    void forward(const TensorInt& inp, TensorInt& lengths, const TensorInt& new_item_indices,
                 TensorInt& decoder_result, int n_new_items, const TensorFloat& emb_table,
                 const TensorFloat& pos_emb_table);
    // EXTENSION: the decoder head draws with these per-slot parameters (DecoderLayer::set_sampling)
    void set_sampling(const SlotSampling* sampling) { decoder_layer_.set_sampling(sampling); }
    // EXTENSION: the sampled head reports log-probabilities into buffers the decoder layer owns (DecoderLayer::set_logprobs)
    void set_logprobs(int n_top) { decoder_layer_.set_logprobs(1, n_top); }
    const DecoderLogprobs& logprobs() const { return decoder_layer_.logprobs(); }

private:
    SelfAttentionLayer attention_layer_;
    EncoderLayer encoder_layer_;
    DecoderLayer decoder_layer_;
    size_t n_batch_, n_sequence_, emb_dim_;
    TensorFloat inp_embedding_;     // [n_batch, n_sequence, emb_dim]
    TensorFloat attention_result_;  // [n_batch, emb_dim]
};

class PagedAttentionInferenceModel : public NonCopyableNonClonable {
public:
    PagedAttentionInferenceModel(PagedAttentionLayer&&, PagedEncoderLayer&&, PagedDecoderLayer&&, size_t n_batch,
                                 size_t n_sequence, size_t emb_dim, int n_forward_rounds);

    // runs n_forward_rounds decode rounds; new rows are only prefilled in round 0
    void forward(const TensorInt& inp, TensorInt& lengths, const TensorInt& new_item_indices,
                 TensorInt& decoder_result, int n_new_items, const TensorFloat& emb_table,
                 const TensorFloat& pos_emb_table, TensorFloatPoint& page_table);
    void set_sampling(const SlotSampling* sampling) { paged_decoder_layer_.set_sampling(sampling); }  // EXTENSION
    void set_logprobs(int n_top) { paged_decoder_layer_.set_logprobs(n_forward_rounds_, n_top); }     // EXTENSION
    const DecoderLogprobs& logprobs() const { return paged_decoder_layer_.logprobs(); }
    void set_n_heads(int n_heads) { paged_attention_layer_.set_n_heads(n_heads); }                    // EXTENSION
    void set_n_kv_heads(int n_kv_heads) { paged_attention_layer_.set_n_kv_heads(n_kv_heads); }        // EXTENSION
    void set_window(int window) { paged_attention_layer_.set_window(window); }                        // EXTENSION
    void set_sinks(int n_sink) { paged_attention_layer_.set_sinks(n_sink); }                          // EXTENSION
    void set_page_release(bool enabled) { paged_attention_layer_.set_page_release(enabled); }         // EXTENSION

private:
    PagedAttentionLayer paged_attention_layer_;
    PagedEncoderLayer paged_encoder_layer_;
    PagedDecoderLayer paged_decoder_layer_;
    size_t n_batch_, n_sequence_, emb_dim_;
    TensorFloat attention_result_;
    int n_forward_rounds_;
    StepGraph decode_graph_;  // replay of the n_new_items == 0 forward (runtime::set_step_graphs)
};

class PagedAttentionCublasInferenceModel : public NonCopyableNonClonable {
public:
    PagedAttentionCublasInferenceModel(PagedAttentionCublasLayer&&, PagedEncoderLayer&&, PagedCublasDecoderLayer&&,
                                       size_t n_batch, size_t n_sequence, size_t emb_dim, int n_forward_rounds);

    void forward(const TensorInt& inp, TensorInt& lengths, const TensorInt& new_item_indices,
                 TensorInt& decoder_result, int n_new_items, const TensorFloat& emb_table,
                 const TensorFloat& pos_emb_table, TensorFloatPoint& page_table, GemmHandle handle);
    void set_sampling(const SlotSampling* sampling) { paged_decoder_layer_.set_sampling(sampling); }  // EXTENSION
    void set_logprobs(int n_top) { paged_decoder_layer_.set_logprobs(n_forward_rounds_, n_top); }     // EXTENSION
    const DecoderLogprobs& logprobs() const { return paged_decoder_layer_.logprobs(); }
    void set_n_heads(int n_heads) { paged_attention_layer_.set_n_heads(n_heads); }                    // EXTENSION
    void set_n_kv_heads(int n_kv_heads) { paged_attention_layer_.set_n_kv_heads(n_kv_heads); }        // EXTENSION
    void set_window(int window) { paged_attention_layer_.set_window(window); }                        // EXTENSION
    void set_sinks(int n_sink) { paged_attention_layer_.set_sinks(n_sink); }                          // EXTENSION
    void set_page_release(bool enabled) { paged_attention_layer_.set_page_release(enabled); }         // EXTENSION

private:
    PagedAttentionCublasLayer paged_attention_layer_;
    PagedEncoderLayer paged_encoder_layer_;
    PagedCublasDecoderLayer paged_decoder_layer_;
    size_t n_batch_, n_sequence_, emb_dim_;
    TensorFloat attention_result_;
    int n_forward_rounds_;
    StepGraph decode_graph_;  // replay of the n_new_items == 0 forward (runtime::set_step_graphs)
};
