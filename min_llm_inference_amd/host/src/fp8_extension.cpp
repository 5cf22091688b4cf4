#include "fp8_extension.h"

#include <utility>

#include "kernels/decoder.h"
#include "mli_kernels.h"
#include "runtime.h"
#include "utils.h"

PagedAttentionFp8Layer::PagedAttentionFp8Layer(TensorBf16&& wk, TensorBf16&& wq, TensorBf16&& wv, size_t n_batch,
                                               size_t emb_dim, size_t n_sequence)
    : PagedAttentionLayerCore(MLI_ELEM_FP8, std::move(wk), std::move(wq), std::move(wv), n_batch, emb_dim, n_sequence) {}

void PagedAttentionFp8Layer::forward(TensorFloatPoint& page_table, const TensorInt& lengths,
                                     const TensorInt& new_batch_idx, TensorFloat& attention_result, int n_new_items) {
    // fp8 pages have the lean composition only: one head, with or without a window and sinks, and nothing to fall back to
    HIP_CHECK(lean_scan(page_table, lengths, new_batch_idx, attention_result, n_new_items, /*n_heads=*/1, /*n_kv_heads=*/0));
}

PagedAttentionFp8InferenceModel::PagedAttentionFp8InferenceModel(PagedAttentionFp8Layer&& attention_layer, size_t n_batch,
                                                                 size_t n_sequence, size_t emb_dim, size_t n_vocab,
                                                                 int n_forward_rounds)
    : PagedInferenceModel(n_batch, n_sequence, emb_dim, n_forward_rounds), attention_layer_(std::move(attention_layer)),
      decoder_head_(n_batch, n_vocab, /*lean_only=*/true) {}

// always the lean layers, whatever runtime::set_lean_layers says (there is no other composition over fp8 pages), and no
// StepGraph (as the bf16 model)
void PagedAttentionFp8InferenceModel::forward_paged(const PagedStep& s, int n_new_items) {
    run_rounds(
        s, n_new_items, /*lean=*/true, attention_layer_, decoder_head_, [](int) {},
        [&](int fresh) { attention_layer_.forward(s.page_table, s.lengths, s.new_item_indices, attention_result_, fresh); });
}
