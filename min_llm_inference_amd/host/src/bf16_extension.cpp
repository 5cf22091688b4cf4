#include "bf16_extension.h"

#include <cstring>
#include <utility>

#include "kernels/decoder.h"
#include "mli_kernels.h"
#include "runtime.h"
#include "utils.h"

namespace {

uint16_t f32_to_bf16_rne(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x40);  // quiet NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return static_cast<uint16_t>(u >> 16);
}

mli_bf16* const* bf16_pages(const TensorFloatPoint& t) { return reinterpret_cast<mli_bf16* const*>(t.data()); }

}  // namespace

TensorBf16 make_device_bf16(const float* host_values, std::vector<size_t> shape) {
    TensorBf16 staging(shape, DeviceType::HOST);
    const size_t n = staging.get_total_size();
    for (size_t i = 0; i < n; ++i) staging.data()[i] = f32_to_bf16_rne(host_values[i]);
    TensorBf16 device(shape, DeviceType::DEVICE);
    device.copy_from(staging);
    return device;
}

void paged_attention_bf16(TensorFloatPoint& page_table, const TensorInt& lengths, const TensorBf16& wk,
                          const TensorBf16& wq, const TensorBf16& wv, const TensorInt& new_batch_idx,
                          TensorFloat& q_output, TensorFloat& qkt_output, TensorFloat& attention_result,
                          int n_new_items, int n_sequence) {
    const int B = (int)page_table.shape()[0], D = (int)wk.shape()[0];
    const mli::runtime::Scratch ws = mli::runtime::attention_scratch(B, n_sequence, D);
    HIP_CHECK(mli_paged_attention_bf16(bf16_pages(page_table), lengths.data(), wk.data(), wq.data(), wv.data(),
                                       new_batch_idx.data(), q_output.data(), qkt_output.data(),
                                       attention_result.data(), B, n_sequence, D, n_new_items,
                                       ws.ptr, ws.bytes, mli::runtime::compute_stream()));
}

void launch_paged_attention_encoder_kernel_bf16(const float* emb_table, const float* wpe, const int* inp,
                                                float** page_table, const int* lengths,
                                                const int* new_item_indices, int batch_size, int n_sequence,
                                                int embedding_dim, int n_new_items) {
    HIP_CHECK(mli_paged_attention_encoder_bf16(emb_table, wpe, inp, reinterpret_cast<mli_bf16* const*>(page_table),
                                               lengths, new_item_indices, batch_size, n_sequence, embedding_dim,
                                               n_new_items, mli::runtime::compute_stream()));
}

void launch_paged_attention_decoder_multi_rounds_bf16(const TensorFloat& batch_result, const TensorFloat& emb_table,
                                                      TensorFloat& emb_score, const TensorFloat& wpe_table,
                                                      TensorFloatPoint& page_table, TensorInt& lengths,
                                                      TensorInt& decoder_result, int i_decoder) {
    const int n_results = decoder_result.shape().size() == 2 ? (int)decoder_result.shape()[1] : 1;
    HIP_CHECK(mli_paged_decoder_multi_rounds_bf16(batch_result.data(), emb_table.data(), emb_score.data(),
                                                  wpe_table.data(), bf16_pages(page_table), lengths.data(),
                                                  decoder_result.data(), (int)batch_result.shape()[0],
                                                  (int)emb_table.shape()[0], (int)wpe_table.shape()[0],
                                                  (int)batch_result.shape()[1], n_results, i_decoder,
                                                  mli::runtime::compute_stream()));
}

PagedAttentionBf16Layer::PagedAttentionBf16Layer(TensorBf16&& wk, TensorBf16&& wq, TensorBf16&& wv, size_t n_batch,
                                                 size_t emb_dim, size_t n_sequence)
    : PagedAttentionLayerCore(MLI_ELEM_BF16, std::move(wk), std::move(wq), std::move(wv), n_batch, emb_dim, n_sequence),
      qkt_output_(std::vector<size_t>{n_batch, n_sequence}, DeviceType::DEVICE) {}

void PagedAttentionBf16Layer::forward(TensorFloatPoint& page_table, const TensorInt& lengths,
                                      const TensorInt& new_batch_idx, TensorFloat& attention_result,
                                      int n_new_items) {
    check_sink_logits();
    check_softcap();
    check_alibi();
    check_rope();
    if (mli::runtime::lean_paged_wanted(options_.n_heads, options_.window, (int)n_sequence_)) {
        const int rc = lean_scan(page_table, lengths, new_batch_idx, attention_result, n_new_items, options_.n_heads,
                                 options_.n_kv_heads);
        if (rc != MLI_ERR_BAD_ARG || wk_.shape()[0] <= 4096) {  // rows wider than the single-pass kernel covers: fall through
            HIP_CHECK(rc);
            return;
        }
    }
    paged_attention_bf16(page_table, lengths, wk_, wq_, wv_, new_batch_idx, q_output_, qkt_output_, attention_result,
                         n_new_items, (int)n_sequence_);
}

PagedAttentionBf16InferenceModel::PagedAttentionBf16InferenceModel(PagedAttentionBf16Layer&& attention_layer,
                                                                   size_t n_batch, size_t n_sequence, size_t emb_dim,
                                                                   size_t n_vocab, int n_forward_rounds)
    : PagedInferenceModel(n_batch, n_sequence, emb_dim, n_forward_rounds), attention_layer_(std::move(attention_layer)),
      decoder_head_(n_batch, n_vocab) {}

// no StepGraph, whatever runtime::set_step_graphs says: graph replay is built and tested for the fp32 and GEMM models only
void PagedAttentionBf16InferenceModel::forward_paged(const PagedStep& s, int n_new_items) {
    run_rounds(
        s, n_new_items, mli::runtime::lean_layers(), attention_layer_, decoder_head_,
        [&](int fresh) {
            launch_paged_attention_encoder_kernel_bf16(s.emb_table.data(), s.pos_emb_table.data(), s.inp.data(),
                                                       s.page_table.data(), s.lengths.data(), s.new_item_indices.data(),
                                                       (int)n_batch_, (int)n_sequence_, (int)emb_dim_, fresh);
        },
        [&](int fresh) { attention_layer_.forward(s.page_table, s.lengths, s.new_item_indices, attention_result_, fresh); });
}
