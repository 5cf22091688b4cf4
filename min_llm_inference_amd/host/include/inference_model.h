// encoder -> attention -> decoder, once per engine iteration (reference include/inference_model.h:8-74).
#pragma once

#include "layers.h"
#include "step_graph.h"
#include "tensor.hpp"
#include "utils.h"

// EXTENSION: what a model forwards to its decoder head, defined once for the contiguous and the paged models.
class DecoderHeadSetters {
public:
    // the decoder head draws with these per-slot parameters (DecoderHead::set_sampling)
    void set_sampling(const SlotSampling* sampling) { decoder_head().set_sampling(sampling); }
    // the sampled head reports log-probabilities into buffers the head owns, one row per forward round
    // (DecoderHead::set_logprobs)
    void set_logprobs(int n_top) { decoder_head().set_logprobs(n_head_rounds_, n_top); }
    const DecoderLogprobs& logprobs() const { return const_cast<DecoderHeadSetters*>(this)->decoder_head().logprobs(); }
    virtual ~DecoderHeadSetters() = default;  // the engine C ABI owns its model through a base pointer

protected:
    explicit DecoderHeadSetters(int n_head_rounds) : n_head_rounds_(n_head_rounds) {}
    virtual DecoderHead& decoder_head() = 0;
    int n_head_rounds_;
};

class InferenceModel : public NonCopyableNonClonable, public DecoderHeadSetters {
public:
    InferenceModel(SelfAttentionLayer&&, EncoderLayer&&, DecoderLayer&&, size_t n_batch, size_t n_sequence,
                   size_t emb_dim);

    void forward(const TensorInt& inp, TensorInt& lengths, const TensorInt& new_item_indices,
                 TensorInt& decoder_result, int n_new_items, const TensorFloat& emb_table,
                 const TensorFloat& pos_emb_table);

private:
    DecoderHead& decoder_head() override { return decoder_layer_; }
    SelfAttentionLayer attention_layer_;
    EncoderLayer encoder_layer_;
    DecoderLayer decoder_layer_;
    size_t n_batch_, n_sequence_, emb_dim_;
    TensorFloat inp_embedding_;     // [n_batch, n_sequence, emb_dim]
    TensorFloat attention_result_;  // [n_batch, emb_dim]
};

// the buffers of one paged forward
struct PagedStep {
    const TensorInt& inp;
    TensorInt& lengths;
    const TensorInt& new_item_indices;
    TensorInt& decoder_result;
    const TensorFloat& emb_table;
    const TensorFloat& pos_emb_table;
    TensorFloatPoint& page_table;
};

// What the four paged models (fp32, GEMM, bf16, fp8) share: the option and decoder-head setters, the rounds loop, and the
// one entry point the engine loops call (inferencer.cpp, pipelined_engine_models.cpp, engine_api.cpp).
class PagedInferenceModel : public NonCopyableNonClonable, public PagedAttentionOptionSetters, public DecoderHeadSetters {
public:
    // runs n_forward_rounds decode rounds; new rows are only prefilled in round 0
    void forward(const TensorInt& inp, TensorInt& lengths, const TensorInt& new_item_indices,
                 TensorInt& decoder_result, int n_new_items, const TensorFloat& emb_table,
                 const TensorFloat& pos_emb_table, TensorFloatPoint& page_table) {
        forward_paged({inp, lengths, new_item_indices, decoder_result, emb_table, pos_emb_table, page_table}, n_new_items);
    }
    // what forward() runs, and what the engine loops call
    virtual void forward_paged(const PagedStep& s, int n_new_items) = 0;

protected:
    PagedInferenceModel(size_t n_batch, size_t n_sequence, size_t emb_dim, int n_forward_rounds)
        : DecoderHeadSetters(n_forward_rounds), n_batch_(n_batch), n_sequence_(n_sequence), emb_dim_(emb_dim),
          attention_result_(std::vector<size_t>{n_batch, emb_dim}, DeviceType::DEVICE),
          n_forward_rounds_(n_forward_rounds) {}

    // n_forward_rounds decode rounds; new rows are only prefilled in round 0.  lean: `layer` prefills (encoder + K/V fill
    // in one launch, the embedding lookup being the fill GEMM's prologue) and attend(0) is a pure decode step; else
    // encode(fresh) and attend(fresh), the reference's two launches -- same pages either way.  A pure decode forward
    // (n_new_items == 0) depends on device state only through the seven buffers of `s`, so a model that passes its
    // StepGraph has it replayed (step_graph.h): the fp32 and the GEMM model do, the bf16 and the fp8 model do not.
    // A template, so that a forward costs the one virtual call of forward_paged.
    template <class Layer, class Encode, class Attend>
    void run_rounds(const PagedStep& s, int n_new_items, bool lean, Layer& layer, DecoderHead& head, Encode&& encode,
                    Attend&& attend, StepGraph* decode_graph = nullptr) {
        auto rounds = [&] {
            for (int round = 0; round < n_forward_rounds_; ++round) {
                const int fresh = round == 0 ? n_new_items : 0;  // later rounds only decode
                // (prompt log-probabilities, layers.h PromptScoring: directly behind the new rows' prefill; a forward with new
                // rows is never a replayed graph)
                if (lean) {
                    layer.prefill(s.emb_table, s.pos_emb_table, s.inp, s.page_table, s.lengths, s.new_item_indices, fresh);
                    if (fresh > 0) layer.score_prompts(s.emb_table, s.inp, s.page_table);
                    attend(0);
                } else {
                    encode(fresh);
                    attend(fresh);
                    if (fresh > 0) layer.score_prompts(s.emb_table, s.inp, s.page_table);
                }
                head.forward_paged(layer.elem(), attention_result_, s.emb_table, s.pos_emb_table, s.page_table, s.lengths,
                                   s.decoder_result, round);
            }
        };
        if (decode_graph == nullptr || n_new_items != 0) return rounds();
        decode_graph->run({s.inp.data(), s.lengths.data(), s.new_item_indices.data(), s.decoder_result.data(),
                           s.emb_table.data(), s.pos_emb_table.data(), s.page_table.data()},
                          rounds);
    }

    size_t n_batch_, n_sequence_, emb_dim_;
    TensorFloat attention_result_;  // [n_batch, emb_dim]
    int n_forward_rounds_;
};

class PagedAttentionInferenceModel : public PagedInferenceModel {
public:
    PagedAttentionInferenceModel(PagedAttentionLayer&&, PagedEncoderLayer&&, PagedDecoderLayer&&, size_t n_batch,
                                 size_t n_sequence, size_t emb_dim, int n_forward_rounds);
    void forward_paged(const PagedStep& s, int n_new_items) override;
    PagedAttentionOptions& options() override { return paged_attention_layer_.options(); }

private:
    DecoderHead& decoder_head() override { return paged_decoder_layer_; }
    PagedAttentionLayer paged_attention_layer_;
    PagedEncoderLayer paged_encoder_layer_;
    PagedDecoderLayer paged_decoder_layer_;
    StepGraph decode_graph_;  // replay of the n_new_items == 0 forward (runtime::set_step_graphs)
};

class PagedAttentionCublasInferenceModel : public PagedInferenceModel {
public:
    PagedAttentionCublasInferenceModel(PagedAttentionCublasLayer&&, PagedEncoderLayer&&, PagedCublasDecoderLayer&&,
                                       size_t n_batch, size_t n_sequence, size_t emb_dim, int n_forward_rounds);
    // the reference's signature; the GemmHandle carries no state, so forward_paged makes its own
    void forward(const TensorInt& inp, TensorInt& lengths, const TensorInt& new_item_indices,
                 TensorInt& decoder_result, int n_new_items, const TensorFloat& emb_table,
                 const TensorFloat& pos_emb_table, TensorFloatPoint& page_table, GemmHandle /*handle*/) {
        forward_paged({inp, lengths, new_item_indices, decoder_result, emb_table, pos_emb_table, page_table}, n_new_items);
    }
    void forward_paged(const PagedStep& s, int n_new_items) override;
    PagedAttentionOptions& options() override { return paged_attention_layer_.options(); }

private:
    DecoderHead& decoder_head() override { return paged_decoder_layer_; }
    PagedAttentionCublasLayer paged_attention_layer_;
    PagedEncoderLayer paged_encoder_layer_;
    PagedCublasDecoderLayer paged_decoder_layer_;
    StepGraph decode_graph_;  // replay of the n_new_items == 0 forward (runtime::set_step_graphs)
};
