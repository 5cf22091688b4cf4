// Greedy decoder head (reference include/kernels/decoder.h:19-37): logits = batch_result . emb_table^T,
// per-row argmax, lengths update (0 when EOF or the row is full), next token's embedding written at
// position lengths[b].
#pragma once

#include <cstdint>
#include <memory>

#include "kernels/paged_attention.h"
#include "tensor.hpp"

void launch_decoder(const TensorFloat& batch_result, const TensorFloat& emb_table, TensorFloat& emb_score,
                    const TensorFloat& wpe_table, TensorFloat& inp_embedding, TensorInt& lengths,
                    TensorInt& decoder_result);

void launch_paged_attention_decoder_multi_rounds(const TensorFloat& batch_result, const TensorFloat& emb_table,
                                                 TensorFloat& emb_score, const TensorFloat& wpe_table,
                                                 TensorFloatPoint& page_table, TensorInt& lengths,
                                                 TensorInt& decoder_result, int i_decoder);

// EXTENSION (no reference counterpart): the same decoder head with the argmax as the logits GEMM's epilogue: same
// tokens, lengths and embeddings; emb_score is lent as scratch and holds no scores afterwards.  What the decoder
// layers run unless runtime::set_lean_layers(false).
void launch_decoder_fused(const TensorFloat& batch_result, const TensorFloat& emb_table, TensorFloat& emb_score,
                          const TensorFloat& wpe_table, TensorFloat& inp_embedding, TensorInt& lengths,
                          TensorInt& decoder_result);
void launch_paged_attention_decoder_fused(const TensorFloat& batch_result, const TensorFloat& emb_table,
                                          TensorFloat& emb_score, const TensorFloat& wpe_table,
                                          TensorFloatPoint& page_table, TensorInt& lengths, TensorInt& decoder_result,
                                          int i_decoder, int elem = 0);  // elem = MLI_ELEM_* of the pages (0: fp32)

// EXTENSION: the sampled decoder head (mli_decoder_sampled / mli_paged_decoder_sampled).  Per-slot device
// arrays [n_batch] of the draw's parameters; a slot with temperature 0 decodes greedily.  emb_score receives the logits.
struct SlotSampling {
    const float* temperature;
    const int* top_k;
    const float* top_p;
    const int64_t* seed;
};
// EXTENSION: per-token log-probabilities beside the sampled head (mli_*_sampled_logprobs).  The device buffers
// a decoder layer owns once set_logprobs was called: token_logprob [n_batch, n_rounds], top_ids / top_logprobs [n_batch,
// n_rounds, n_top], strided like decoder_result and at fixed addresses (step graphs replay them).  Sync flavour like the
// engine's other per-slot arrays: they cross to the host by stream-ordered copies.
struct DecoderLogprobs {
    int n_top = -1;  // -1: off
    int n_rounds = 1;
    std::unique_ptr<TensorFloat> token_logprob, top_logprobs;
    std::unique_ptr<TensorInt> top_ids;

    bool on() const { return n_top >= 0; }
    void allocate(size_t n_batch, size_t rounds, int top) {
        const size_t width = top > 0 ? (size_t)top : 1;  // n_top == 0: the lists are never written
        constexpr TensorDataType kSync = TensorDataType::SYNC_ALLOCATE;
        token_logprob = std::make_unique<TensorFloat>(std::vector<size_t>{n_batch, rounds}, DeviceType::DEVICE, kSync);
        top_logprobs = std::make_unique<TensorFloat>(std::vector<size_t>{n_batch, rounds, width}, DeviceType::DEVICE, kSync);
        top_ids = std::make_unique<TensorInt>(std::vector<size_t>{n_batch, rounds, width}, DeviceType::DEVICE, kSync);
        n_top = top;
        n_rounds = (int)rounds;
    }
};

// logprobs: nullptr or off = the plain sampled head (the same code objects as before the extension)
void launch_decoder_sampled(const TensorFloat& batch_result, const TensorFloat& emb_table, TensorFloat& emb_score,
                            const TensorFloat& wpe_table, TensorFloat& inp_embedding, TensorInt& lengths,
                            TensorInt& decoder_result, const SlotSampling& sampling,
                            const DecoderLogprobs* logprobs = nullptr);
// elem = MLI_ELEM_* of the pages
void launch_paged_attention_decoder_sampled(const TensorFloat& batch_result, const TensorFloat& emb_table,
                                            TensorFloat& emb_score, const TensorFloat& wpe_table,
                                            TensorFloatPoint& page_table, TensorInt& lengths, TensorInt& decoder_result,
                                            int i_decoder, int elem, const SlotSampling& sampling,
                                            const DecoderLogprobs* logprobs = nullptr);

void launch_paged_attention_cublas_decoder_multi_rounds(const TensorFloat& batch_result,
                                                        const TensorFloat& emb_table, TensorFloat& emb_score,
                                                        const TensorFloat& wpe_table, TensorFloatPoint& page_table,
                                                        TensorInt& lengths, TensorInt& decoder_result, int i_decoder,
                                                        GemmHandle& handle);
