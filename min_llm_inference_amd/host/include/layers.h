// Layer objects: own the weights and the pre-allocated scratch, unpack shapes, call the launchers.
// Same constructors and forward() signatures as the reference (include/layers.h:19-156) for the layers
// on the inference path.  FeedForward (used by no model in the reference) is out of scope.
#pragma once

#include <cstdint>
#include <memory>
#include <vector>

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

// EXTENSION: the options of the paged attention layers' lean forward, one struct for the four layers and the four models.
// A new per-layer option is a field here, its setter below, one validation in the engine setter (engine_api.cpp) and its
// use where the layer launches (layers.cpp).
// EXTENSION: prompt log-probabilities.  What a layer calls right after the prefill of a forward's new rows, on
// the forward's stream, with its own projection weights and options: the engine's scorer (engine_api.cpp) cuts the new rows'
// prompts into passes and runs mli_paged_prompt_logprobs on each.  A forward without new rows never calls it.
struct PagedAttentionOptions;
struct PromptScoring {
    virtual ~PromptScoring() = default;
    virtual void score(int elem, const void* wq, const PagedAttentionOptions& options, void* const* page_table, const int* inp,
                       const float* emb_table, int n_batch, int n_sequence, int emb_dim, int n_vocab) = 0;
};

struct PagedAttentionOptions {
    int n_heads = 1;            // attention heads (1 = the reference's single softmax over emb_dim)
    int n_kv_heads = 0;         // grouped-query attention: K/V heads serving the n_heads query heads (0 = as many)
    int window = 0;             // sliding window: a row attends its newest `window` tokens (0 or >= n_sequence: all)
    int n_sink = 0;             // attention sinks: beside a window a row keeps its first n_sink tokens attended (0: none)
    // the rows' pages below the window are returned early (PagedAttentionsManager::set_page_release): prefill covers a
    // row's live tokens only and follows no table entry of a dead page (mli_paged_prefill_window)
    bool page_release = false;
    PromptScoring* prompt_logprobs = nullptr;   // prompt log-probabilities: who scores the new rows' prompts (nullptr: nobody)
    // ALiBi: one slope per query head ([n_heads], device memory, owned here; null: no bias) -- mli_paged_attention_lean_alibi
    std::shared_ptr<TensorFloat> alibi_slopes;
    // Rotary position embeddings: [n_sequence][head_dim / 2] (cos, sin) pairs (device memory, owned here; null: none) --
    // mli_paged_prefill_rope, mli_paged_attention_lean_rope.  n_sequence and emb_dim are the layer's, set by its constructor:
    // set_rope sizes the table by them.
    std::shared_ptr<TensorFloat> rope_table;
    int n_sequence = 0, emb_dim = 0;
    // Logit soft-capping: every scaled attention score x becomes softcap * tanh(x / softcap), in the decode scan and in the
    // prompt scan (0: none) -- mli_paged_attention_lean_softcap, mli_paged_prompt_logprobs_softcap
    float softcap = 0.f;
    // Learned attention-sink logits: one per query head ([n_heads], device memory at a fixed address, owned here; null: none),
    // one more logit of the head's softmax without a value row, in the decode scan and in the prompt scan --
    // mli_paged_attention_lean_sink_logits, mli_paged_prompt_logprobs_sink_logits
    std::shared_ptr<TensorFloat> sink_logits;
};

// The setters of the option set, defined once for every class that has them: a layer owns the struct, a model hands out
// its layer's.  A class whose scan has one head only (fp8 pages) takes set_n_heads / set_n_kv_heads / set_alibi_slopes /
// set_softcap / set_sink_logits out of its interface.
class PagedAttentionOptionSetters {
public:
    // EXTENSION: ALiBi -- slopes[h] * (s - (L - 1)) added to query head h's scaled scores; n_heads finite values, uploaded
    // to a device copy the option set owns.  An empty vector takes the bias away again.  A non-finite slope throws here; the
    // count is held to n_heads (>= 2) at every forward, whichever setter came last (PagedAttentionLayerCore::check_alibi).
    void set_alibi_slopes(const std::vector<float>& slopes);
    // EXTENSION: rotary position embeddings -- prefill and projection rotate K (before its one rounding) and q by the token's
    // absolute slot (include/mli_kernels.h).  set_rope builds the standard table (mli_rope_table) for the CURRENT n_heads at the
    // layer's n_sequence: set the heads first.  set_rope_table takes any table, n_sequence * head_dim finite floats ((cos, sin)
    // pairs; the scaled variants are just another table); an empty vector takes the rotation away again.  Either uploads a
    // device copy the option set owns.  The count is held to n_sequence * head_dim at every forward, whichever setter came
    // last (PagedAttentionLayerCore::check_rope).
    void set_rope(double theta);
    void set_rope_table(const std::vector<float>& table);
    // EXTENSION: attention logit soft-capping -- cap * tanh(x / cap) on every scaled score of the decode scan and of the prompt
    // scan; 0 takes the cap away again.  A negative or non-finite cap throws here; two heads at least, the lean layers and no
    // slopes beside it are held at every forward, whichever setter came last (PagedAttentionLayerCore::check_softcap).
    void set_softcap(float cap);
    // EXTENSION: learned attention-sink logits -- host[h] joins query head h's softmax as one more logit without a value row
    // (maximum and denominator, once per row and head), in the decode scan and in the prompt scan.  n values, each finite or
    // -inf (-inf: no sink for that head), uploaded to a device copy the option set owns: its address stays fixed, so a captured
    // step graph replays it.  host null or n == 0 takes the switch away again.  NaN or +inf throws here; the count is held to
    // n_heads (>= 2), the lean layers and neither slopes nor a cap beside it at every forward, whichever setter came last
    // (PagedAttentionLayerCore::check_sink_logits).
    void set_sink_logits(const float* host, int n);
    void set_n_heads(int n_heads) { options().n_heads = n_heads; }
    void set_n_kv_heads(int n_kv_heads) { options().n_kv_heads = n_kv_heads; }
    void set_window(int window) { options().window = window; }
    void set_sinks(int n_sink) { options().n_sink = n_sink; }
    void set_page_release(bool enabled) { options().page_release = enabled; }
    void set_prompt_logprobs(PromptScoring* scoring) { options().prompt_logprobs = scoring; }
    virtual PagedAttentionOptions& options() = 0;

protected:
    ~PagedAttentionOptionSetters() = default;
};

// What the paged attention layers of every page element type share: weights, the q scratch, the option set, the fused
// prefill and the lean scan.  Weights = TensorFloat (fp32 pages) or Tensor<uint16_t> (bf16 weights: bf16 and fp8 pages).
template <class Weights>
class PagedAttentionLayerCore : public NonCopyableNonClonable, public PagedAttentionOptionSetters {
public:
    // extension: encoder + K/V prefill of the new rows in one launch (the model then calls forward with n_new_items = 0);
    // n_new_items == 0 launches nothing
    void prefill(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                 TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_item_indices,
                 int n_new_items);
    // extension: the prompt log-probabilities of the rows just prefilled (PromptScoring); nothing without a scorer
    void score_prompts(const TensorFloat& emb_table, const TensorInt& inp, TensorFloatPoint& page_table);
    PagedAttentionOptions& options() override { return options_; }
    int elem() const { return elem_; }  // MLI_ELEM_* of the pages

protected:
    PagedAttentionLayerCore(int elem, Weights&& wk, Weights&& wq, Weights&& wv, size_t n_batch, size_t emb_dim,
                            size_t n_sequence);
    // runtime::lean_paged_attention over this layer's pages and options; its status comes back because what a layer does
    // with rows too wide for the single-pass kernel differs by element type
    int lean_scan(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_batch_idx,
                  TensorFloat& attention_result, int n_new_items, int n_heads, int n_kv_heads);
    // throws where slopes are set and are not one per head of n_heads >= 2 heads, or the lean layers are off: first thing in
    // every forward, so that no scan reads past the slopes and no composition without a bias drops them
    void check_alibi() const;
    // throws where a rotary table is set and is not n_sequence * head_dim floats for an even head_dim = emb_dim / n_heads, or
    // the lean layers are off (the materialising compositions have no rotation): first thing in every prefill and forward
    void check_rope() const;
    // throws where a cap is set beside n_heads < 2, the lean layers off (the materialising composition has no cap and must
    // never drop it silently) or ALiBi slopes (no order of bias and cap is defined): first thing in every forward
    void check_softcap() const;
    // throws where sink logits are set and are not one per head of n_heads >= 2 heads, the lean layers are off (the
    // materialising composition has no sink logit and must never drop it silently), or ALiBi slopes or a cap stand beside them
    // (no model defines that): first thing in every forward
    void check_sink_logits() const;

    int elem_;
    Weights wk_, wq_, wv_;
    TensorFloat q_output_;
    size_t n_sequence_;
    PagedAttentionOptions options_;
};
extern template class PagedAttentionLayerCore<TensorFloat>;
extern template class PagedAttentionLayerCore<Tensor<uint16_t>>;

// PagedAttentionLayer and PagedAttentionCublasLayer are one layer but for the materialising composition they run with the
// lean layers off (and for rows too wide for the lean scan).
class PagedAttentionFloatLayer : public PagedAttentionLayerCore<TensorFloat> {
protected:
    PagedAttentionFloatLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch, size_t emb_dim,
                             size_t n_sequence);
    // true: the lean composition ran.  false: the caller runs its materialising composition into qkt_output_ -- the lean
    // layers are off, or the scan refused one head without a window with MLI_ERR_BAD_ARG for emb_dim > 2048, % 4 == 0
    bool forward_lean(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_batch_idx,
                      TensorFloat& attention_result, int n_new_items);
    TensorFloat qkt_output_;
};

class PagedAttentionLayer : public PagedAttentionFloatLayer {
public:
    PagedAttentionLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch, size_t emb_dim,
                        size_t n_sequence);
    void forward(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_batch_idx,
                 TensorFloat& attention_result, int n_new_items);
};

class PagedAttentionCublasLayer : public PagedAttentionFloatLayer {
public:
    PagedAttentionCublasLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch, size_t emb_dim,
                              size_t n_sequence);
    void forward(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorInt& new_batch_idx,
                 TensorFloat& attention_result, int n_new_items, GemmHandle& handle);

private:
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

// What the three decoder layers and the bf16 / fp8 models hold of a decoder head: the logits buffer, the sampling
// parameters, the log-probability buffers, and the one choice between the sampled, the lean and the materialising head.
class DecoderHead : public NonCopyableNonClonable {
public:
    // lean_only (fp8 pages, which have no materialising head): the lean head's scratch (mli_decoder_scratch_bytes) is
    // all that is allocated, and emb_score [n_batch, n_vocab] follows when set_sampling asks for the sampled head
    DecoderHead(size_t n_batch, size_t n_vocab, bool lean_only = false);

    // EXTENSION: from now on forward() runs the sampled head with these per-slot parameters (nullptr: the greedy head)
    void set_sampling(const SlotSampling* sampling);
    // EXTENSION: the sampled head also reports log-probabilities into buffers this head owns from now on:
    // [n_batch, n_rounds(, n_top)], n_top in 0 .. 8.  Takes effect where the sampled head runs (set_sampling).
    void set_logprobs(int n_rounds, int n_top) { logprobs_.allocate(n_batch_, (size_t)n_rounds, n_top); }
    const DecoderLogprobs& logprobs() const { return logprobs_; }

    // The head of one round over pages of elem = MLI_ELEM_*: sampled (with or without log-probabilities) if set_sampling
    // gave parameters, else the lean fused head, else -- lean layers off -- the element type's materialising head.
    void forward_paged(int elem, const TensorFloat& batch_result, const TensorFloat& emb_table,
                       const TensorFloat& wpe_table, TensorFloatPoint& page_table, TensorInt& lengths,
                       TensorInt& decoder_result, int i_decoder_round);

protected:
    size_t n_batch_, n_vocab_;
    std::unique_ptr<TensorFloat> emb_score_;     // [n_batch, n_vocab]; lent to the lean head as scratch
    std::unique_ptr<TensorFloat> lean_scratch_;  // a lean_only head's scratch instead
    const SlotSampling* sampling_ = nullptr;
    DecoderLogprobs logprobs_;
};

class DecoderLayer : public DecoderHead {
public:
    DecoderLayer(size_t n_batch, size_t n_vocab) : DecoderHead(n_batch, n_vocab) {}
    void forward(const TensorFloat& batch_result, const TensorFloat& emb_table, const TensorFloat& wpe_table,
                 TensorFloat& inp_embedding, TensorInt& lengths, TensorInt& decoder_result);
};

class PagedDecoderLayer : public DecoderHead {
public:
    PagedDecoderLayer(size_t n_batch, size_t n_vocab) : DecoderHead(n_batch, n_vocab) {}
    void forward(const TensorFloat& batch_result, const TensorFloat& emb_table, const TensorFloat& wpe_table,
                 TensorFloatPoint& page_table, TensorInt& lengths, TensorInt& decoder_result, int i_decoder_round);
};

class PagedCublasDecoderLayer : public DecoderHead {
public:
    PagedCublasDecoderLayer(size_t n_batch, size_t n_vocab) : DecoderHead(n_batch, n_vocab) {}
    void forward(const TensorFloat& batch_result, const TensorFloat& emb_table, const TensorFloat& wpe_table,
                 TensorFloatPoint& page_table, TensorInt& lengths, TensorInt& decoder_result, int i_decoder_round,
                 GemmHandle& handle);
};
