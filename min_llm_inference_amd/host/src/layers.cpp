#include "layers.h"

#include <algorithm>
#include <cmath>
#include <stdexcept>
#include <string>
#include <utility>

#include "bf16_extension.h"  // launch_paged_attention_decoder_multi_rounds_bf16
#include "kernels/decoder.h"
#include "kernels/encoder.h"
#include "kernels/paged_attention.h"
#include "kernels/self_attention_inference_optimized.h"
#include "mli_kernels.h"
#include "runtime.h"

namespace {
TensorFloat device_tensor(std::initializer_list<size_t> shape) {
    return TensorFloat(std::vector<size_t>(shape), DeviceType::DEVICE);
}
}  // namespace

SelfAttentionLayer::SelfAttentionLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch,
                                       size_t input_dim, size_t n_sequence)
    : wk_(std::move(wk)), wq_(std::move(wq)), wv_(std::move(wv)),
      kt_cache_(device_tensor({n_batch, input_dim, n_sequence})),
      v_cache_(device_tensor({n_batch, n_sequence, input_dim})),
      q_output_(device_tensor({n_batch, input_dim})),
      qkt_output_(device_tensor({n_batch, n_sequence})) {}

void SelfAttentionLayer::forward(const TensorFloat& inp_embedding, const TensorInt& lengths,
                                 const TensorInt& new_batch_idx, TensorFloat& attention_result, int n_new_items) {
    if (mli::runtime::lean_layers())
        inference_self_attention_lean(inp_embedding, lengths, wk_, wq_, wv_, new_batch_idx, kt_cache_, v_cache_, q_output_,
                                      qkt_output_, attention_result, n_new_items);
    else
        inference_self_attention(inp_embedding, lengths, wk_, wq_, wv_, new_batch_idx, kt_cache_, v_cache_, q_output_,
                                 qkt_output_, attention_result, n_new_items);
}

void SelfAttentionLayer::prefill(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                                 TensorFloat& inp_embedding, const TensorInt& lengths,
                                 const TensorInt& new_item_indices, int n_new_items) {
    launch_prefill(emb_table, pos_emb, inp, inp_embedding, lengths, new_item_indices, wk_, wv_, kt_cache_, v_cache_,
                   n_new_items);
}

void PagedAttentionOptionSetters::set_alibi_slopes(const std::vector<float>& slopes) {
    if (slopes.empty()) {
        options().alibi_slopes.reset();
        return;
    }
    for (float s : slopes)
        if (!std::isfinite(s)) throw std::invalid_argument("set_alibi_slopes: every slope must be finite");
    TensorFloat host(std::vector<size_t>{slopes.size()}, DeviceType::HOST, TensorDataType::SYNC_ALLOCATE);
    std::copy(slopes.begin(), slopes.end(), host.data());
    auto device = std::make_shared<TensorFloat>(std::vector<size_t>{slopes.size()}, DeviceType::DEVICE, TensorDataType::SYNC_ALLOCATE);
    device->copy_from(host);
    options().alibi_slopes = std::move(device);
}

void PagedAttentionOptionSetters::set_softcap(float cap) {
    if (!std::isfinite(cap) || cap < 0.f) throw std::invalid_argument("set_softcap: the cap must be finite and >= 0 (0: none)");
    options().softcap = cap;
}

void PagedAttentionOptionSetters::set_sink_logits(const float* values, int n) {
    if (values == nullptr || n == 0) {
        options().sink_logits.reset();
        return;
    }
    if (n < 0) throw std::invalid_argument("set_sink_logits: a negative count");
    for (int h = 0; h < n; ++h)
        if (std::isnan(values[h]) || values[h] == INFINITY)
            throw std::invalid_argument("set_sink_logits: every logit must be finite or -inf (NaN and +inf are refused)");
    TensorFloat host(std::vector<size_t>{(size_t)n}, DeviceType::HOST, TensorDataType::SYNC_ALLOCATE);
    std::copy(values, values + n, host.data());
    auto device = std::make_shared<TensorFloat>(std::vector<size_t>{(size_t)n}, DeviceType::DEVICE, TensorDataType::SYNC_ALLOCATE);
    device->copy_from(host);
    options().sink_logits = std::move(device);
}

void PagedAttentionOptionSetters::set_rope_table(const std::vector<float>& table) {
    if (table.empty()) {
        options().rope_table.reset();
        return;
    }
    for (float t : table)
        if (!std::isfinite(t)) throw std::invalid_argument("set_rope_table: every entry must be finite");
    TensorFloat host(std::vector<size_t>{table.size()}, DeviceType::HOST, TensorDataType::SYNC_ALLOCATE);
    std::copy(table.begin(), table.end(), host.data());
    auto device = std::make_shared<TensorFloat>(std::vector<size_t>{table.size()}, DeviceType::DEVICE, TensorDataType::SYNC_ALLOCATE);
    device->copy_from(host);
    options().rope_table = std::move(device);
}

void PagedAttentionOptionSetters::set_rope(double theta) {
    const PagedAttentionOptions& o = options();
    if (o.n_heads < 1 || o.emb_dim < 1 || o.n_sequence < 1 || o.emb_dim % o.n_heads != 0)
        throw std::invalid_argument("set_rope: emb_dim " + std::to_string(o.emb_dim) + " is no multiple of n_heads " +
                                    std::to_string(o.n_heads));
    const int hd = o.emb_dim / o.n_heads;
    std::vector<float> table(hd % 2 == 0 ? (size_t)o.n_sequence * hd : 0);
    if (table.empty() || mli_rope_table(o.n_sequence, hd, theta, table.data()) != 0)
        throw std::invalid_argument("set_rope: head_dim must be even and theta finite and > 0");
    set_rope_table(table);
}

template <class Weights>
PagedAttentionLayerCore<Weights>::PagedAttentionLayerCore(int elem, Weights&& wk, Weights&& wq, Weights&& wv,
                                                          size_t n_batch, size_t emb_dim, size_t n_sequence)
    : elem_(elem), wk_(std::move(wk)), wq_(std::move(wq)), wv_(std::move(wv)),
      q_output_(device_tensor({n_batch, emb_dim})), n_sequence_(n_sequence) {
    options_.n_sequence = (int)n_sequence;
    options_.emb_dim = (int)emb_dim;
}

template <class Weights>
void PagedAttentionLayerCore<Weights>::prefill(const TensorFloat& emb_table, const TensorFloat& pos_emb,
                                               const TensorInt& inp, TensorFloatPoint& page_table,
                                               const TensorInt& lengths, const TensorInt& new_item_indices,
                                               int n_new_items) {
    check_rope();
    launch_paged_prefill_elem(emb_table, pos_emb, inp, page_table, lengths, new_item_indices, wk_.data(), wv_.data(),
                              n_new_items, elem_, options_.page_release, options_.window, options_.n_sink, options_.n_heads,
                              options_.rope_table ? options_.rope_table->data() : nullptr);
}

template <class Weights>
void PagedAttentionLayerCore<Weights>::score_prompts(const TensorFloat& emb_table, const TensorInt& inp,
                                                     TensorFloatPoint& page_table) {
    if (options_.prompt_logprobs == nullptr) return;
    options_.prompt_logprobs->score(elem_, wq_.data(), options_, reinterpret_cast<void* const*>(page_table.data()), inp.data(),
                                    emb_table.data(), (int)page_table.shape()[0], (int)n_sequence_, (int)wk_.shape()[0],
                                    (int)emb_table.shape()[0]);
}

// The setters come in any order, so the slopes are held to the heads where they are used: at every forward, before anything
// is launched.  n_heads >= 2 with lean layers off has thrown already (lean_paged_wanted); one head would take the
// materialising composition, which has no bias, so slopes beside one head throw here instead of being dropped.
template <class Weights>
void PagedAttentionLayerCore<Weights>::check_alibi() const {
    if (!options_.alibi_slopes) return;
    if (options_.n_heads < 2 || options_.alibi_slopes->get_total_size() != (size_t)options_.n_heads)
        throw std::runtime_error("ALiBi: " + std::to_string(options_.alibi_slopes->get_total_size()) + " slopes (set_alibi_slopes) "
                                 "beside n_heads = " + std::to_string(options_.n_heads) + ": one slope per head, two heads at least");
    if (!mli::runtime::lean_layers()) throw std::runtime_error("ALiBi exists in the lean composition only");
}

// As check_alibi: the setters come in any order, so the table is held to the heads where it is used.  A layer with a table and
// the lean layers off throws: the materialising compositions (and an encoder launch of its own) have no rotation.
template <class Weights>
void PagedAttentionLayerCore<Weights>::check_rope() const {
    if (!options_.rope_table) return;
    const size_t D = wk_.shape()[0], H = (size_t)std::max(options_.n_heads, 1);
    if (D % H != 0 || (D / H) % 2 != 0 || options_.rope_table->get_total_size() != n_sequence_ * (D / H))
        throw std::runtime_error("RoPE: a table of " + std::to_string(options_.rope_table->get_total_size()) +
                                 " floats (set_rope / set_rope_table) beside n_heads = " + std::to_string(options_.n_heads) +
                                 ": n_sequence * head_dim floats for an even head_dim = emb_dim / n_heads");
    if (!mli::runtime::lean_layers()) throw std::runtime_error("RoPE exists in the lean composition only");
}

// As check_alibi.  One head would take the single-head scans or the materialising composition, which have no cap: a cap beside
// one head, or with the lean layers off, throws here instead of being dropped.
template <class Weights>
void PagedAttentionLayerCore<Weights>::check_softcap() const {
    if (options_.softcap == 0.f) return;
    if (options_.n_heads < 2)
        throw std::runtime_error("logit soft-capping (set_softcap) beside n_heads = " + std::to_string(options_.n_heads) +
                                 ": two heads at least");
    if (!mli::runtime::lean_layers()) throw std::runtime_error("logit soft-capping exists in the lean composition only");
    if (options_.alibi_slopes)
        throw std::runtime_error("logit soft-capping (set_softcap) and ALiBi (set_alibi_slopes) are not combined");
}

// As check_alibi: the logits are held to the heads where they are used, and never dropped by a composition without them.
template <class Weights>
void PagedAttentionLayerCore<Weights>::check_sink_logits() const {
    if (!options_.sink_logits) return;
    if (options_.n_heads < 2 || options_.sink_logits->get_total_size() != (size_t)options_.n_heads)
        throw std::runtime_error("attention-sink logits: " + std::to_string(options_.sink_logits->get_total_size()) +
                                 " logits (set_sink_logits) beside n_heads = " + std::to_string(options_.n_heads) +
                                 ": one logit per head, two heads at least");
    if (!mli::runtime::lean_layers()) throw std::runtime_error("attention-sink logits exist in the lean composition only");
    if (options_.alibi_slopes)
        throw std::runtime_error("attention-sink logits (set_sink_logits) and ALiBi (set_alibi_slopes) are not combined");
    if (options_.softcap != 0.f)
        throw std::runtime_error("attention-sink logits (set_sink_logits) and logit soft-capping (set_softcap) are not combined");
}

template <class Weights>
int PagedAttentionLayerCore<Weights>::lean_scan(TensorFloatPoint& page_table, const TensorInt& lengths,
                                                const TensorInt& new_batch_idx, TensorFloat& attention_result,
                                                int n_new_items, int n_heads, int n_kv_heads) {
    check_sink_logits();
    check_softcap();
    check_alibi();
    check_rope();
    return mli::runtime::lean_paged_attention(elem_, n_heads, options_.window, options_.n_sink,
                                              reinterpret_cast<void* const*>(page_table.data()), lengths.data(),
                                              wk_.data(), wq_.data(), wv_.data(), new_batch_idx.data(), q_output_.data(),
                                              attention_result.data(), (int)page_table.shape()[0], (int)n_sequence_,
                                              (int)wk_.shape()[0], n_new_items, n_kv_heads,
                                              options_.alibi_slopes ? options_.alibi_slopes->data() : nullptr,
                                              options_.rope_table ? options_.rope_table->data() : nullptr, options_.softcap,
                                              options_.sink_logits ? options_.sink_logits->data() : nullptr);
}

template class PagedAttentionLayerCore<TensorFloat>;
template class PagedAttentionLayerCore<Tensor<uint16_t>>;

PagedAttentionFloatLayer::PagedAttentionFloatLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch,
                                                   size_t emb_dim, size_t n_sequence)
    : PagedAttentionLayerCore(MLI_ELEM_F32, std::move(wk), std::move(wq), std::move(wv), n_batch, emb_dim, n_sequence),
      qkt_output_(device_tensor({n_batch, n_sequence})) {}

bool PagedAttentionFloatLayer::forward_lean(TensorFloatPoint& page_table, const TensorInt& lengths,
                                            const TensorInt& new_batch_idx, TensorFloat& attention_result,
                                            int n_new_items) {
    check_sink_logits();
    check_softcap();
    check_alibi();
    check_rope();
    if (!mli::runtime::lean_paged_wanted(options_.n_heads, options_.window, (int)n_sequence_)) return false;
    const int rc = lean_scan(page_table, lengths, new_batch_idx, attention_result, n_new_items, options_.n_heads,
                             options_.n_kv_heads);
    const int D = (int)wk_.shape()[0];
    if (rc == MLI_ERR_BAD_ARG && D > 2048 && D % 4 == 0) return false;  // rows wider than the single-pass kernel covers
    HIP_CHECK(rc);
    return true;
}

PagedAttentionLayer::PagedAttentionLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv, size_t n_batch,
                                         size_t emb_dim, size_t n_sequence)
    : PagedAttentionFloatLayer(std::move(wk), std::move(wq), std::move(wv), n_batch, emb_dim, n_sequence) {}

void PagedAttentionLayer::forward(TensorFloatPoint& page_table, const TensorInt& lengths,
                                  const TensorInt& new_batch_idx, TensorFloat& attention_result, int n_new_items) {
    if (!forward_lean(page_table, lengths, new_batch_idx, attention_result, n_new_items))
        paged_attention(page_table, lengths, wk_, wq_, wv_, new_batch_idx, q_output_, qkt_output_, attention_result,
                        n_new_items, (int)n_sequence_);
}

PagedAttentionCublasLayer::PagedAttentionCublasLayer(TensorFloat&& wk, TensorFloat&& wq, TensorFloat&& wv,
                                                     size_t n_batch, size_t emb_dim, size_t n_sequence)
    : PagedAttentionFloatLayer(std::move(wk), std::move(wq), std::move(wv), n_batch, emb_dim, n_sequence),
      latest_emb_(device_tensor({n_batch, emb_dim})),
      temp_placeholder_(device_tensor({n_batch, emb_dim})) {}

void PagedAttentionCublasLayer::forward(TensorFloatPoint& page_table, const TensorInt& lengths,
                                        const TensorInt& new_batch_idx, TensorFloat& attention_result,
                                        int n_new_items, GemmHandle& handle) {
    if (!forward_lean(page_table, lengths, new_batch_idx, attention_result, n_new_items))
        paged_attention_with_cublas(page_table, lengths, wk_, wq_, wv_, new_batch_idx, q_output_, qkt_output_,
                                    attention_result, latest_emb_, temp_placeholder_, n_new_items, (int)n_sequence_, handle);
}

void EncoderLayer::forward(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                           TensorFloat& inp_embedding, const TensorInt& lengths, const TensorInt& new_item_indices,
                           int n_new_items) {
    const auto& s = inp_embedding.shape();
    launch_inference_optimized_encoder_kernel(emb_table.data(), pos_emb.data(), inp.data(), inp_embedding.data(),
                                              lengths.data(), new_item_indices.data(), static_cast<int>(s[0]),
                                              static_cast<int>(s[1]), static_cast<int>(s[2]), n_new_items);
}

void PagedEncoderLayer::forward(const TensorFloat& emb_table, const TensorFloat& pos_emb, const TensorInt& inp,
                                TensorFloatPoint& page_table, const TensorInt& lengths,
                                const TensorInt& new_item_indices, int n_new_items) {
    launch_paged_attention_encoder_kernel(emb_table.data(), pos_emb.data(), inp.data(), page_table.data(),
                                          lengths.data(), new_item_indices.data(), static_cast<int>(inp.shape()[0]),
                                          static_cast<int>(inp.shape()[1]), static_cast<int>(emb_table.shape()[1]),
                                          n_new_items);
}

DecoderHead::DecoderHead(size_t n_batch, size_t n_vocab, bool lean_only) : n_batch_(n_batch), n_vocab_(n_vocab) {
    if (lean_only)
        lean_scratch_ = std::make_unique<TensorFloat>(device_tensor({(mli_decoder_scratch_bytes((int)n_batch, (int)n_vocab) + 3) / 4}));
    else
        emb_score_ = std::make_unique<TensorFloat>(device_tensor({n_batch, n_vocab}));
}

void DecoderHead::set_sampling(const SlotSampling* sampling) {
    if (sampling && !emb_score_) emb_score_ = std::make_unique<TensorFloat>(device_tensor({n_batch_, n_vocab_}));
    sampling_ = sampling;
}

void DecoderHead::forward_paged(int elem, const TensorFloat& batch_result, const TensorFloat& emb_table,
                                const TensorFloat& wpe_table, TensorFloatPoint& page_table, TensorInt& lengths,
                                TensorInt& decoder_result, int i_decoder_round) {
    if (sampling_)
        launch_paged_attention_decoder_sampled(batch_result, emb_table, *emb_score_, wpe_table, page_table, lengths,
                                               decoder_result, i_decoder_round, elem, *sampling_, &logprobs_);
    else if (lean_scratch_ || mli::runtime::lean_layers())  // a lean_only head does not read the switch
        launch_paged_attention_decoder_fused(batch_result, emb_table, lean_scratch_ ? *lean_scratch_ : *emb_score_,
                                             wpe_table, page_table, lengths, decoder_result, i_decoder_round, elem);
    else if (elem == MLI_ELEM_BF16)
        launch_paged_attention_decoder_multi_rounds_bf16(batch_result, emb_table, *emb_score_, wpe_table, page_table,
                                                         lengths, decoder_result, i_decoder_round);
    else
        launch_paged_attention_decoder_multi_rounds(batch_result, emb_table, *emb_score_, wpe_table, page_table, lengths,
                                                    decoder_result, i_decoder_round);
}

void DecoderLayer::forward(const TensorFloat& batch_result, const TensorFloat& emb_table,
                           const TensorFloat& wpe_table, TensorFloat& inp_embedding, TensorInt& lengths,
                           TensorInt& decoder_result) {
    if (sampling_)
        launch_decoder_sampled(batch_result, emb_table, *emb_score_, wpe_table, inp_embedding, lengths, decoder_result,
                               *sampling_, &logprobs_);
    else if (mli::runtime::lean_layers())
        launch_decoder_fused(batch_result, emb_table, *emb_score_, wpe_table, inp_embedding, lengths, decoder_result);
    else
        launch_decoder(batch_result, emb_table, *emb_score_, wpe_table, inp_embedding, lengths, decoder_result);
}

void PagedDecoderLayer::forward(const TensorFloat& batch_result, const TensorFloat& emb_table,
                                const TensorFloat& wpe_table, TensorFloatPoint& page_table, TensorInt& lengths,
                                TensorInt& decoder_result, int i_decoder_round) {
    forward_paged(MLI_ELEM_F32, batch_result, emb_table, wpe_table, page_table, lengths, decoder_result, i_decoder_round);
}

// the "cuBLAS" materialising head is the plain one (launch_paged_attention_cublas_decoder_multi_rounds, launchers.cpp)
void PagedCublasDecoderLayer::forward(const TensorFloat& batch_result, const TensorFloat& emb_table,
                                      const TensorFloat& wpe_table, TensorFloatPoint& page_table,
                                      TensorInt& lengths, TensorInt& decoder_result, int i_decoder_round,
                                      GemmHandle& /*handle*/) {
    forward_paged(MLI_ELEM_F32, batch_result, emb_table, wpe_table, page_table, lengths, decoder_result, i_decoder_round);
}
