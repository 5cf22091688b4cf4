// The causal multi-query prompt scan on matrix instructions over bf16 pages, and its entry points: attention_prompt_mfma.hpp
// has the account and the kernel.  Five kernels (head_dim 64 with 1 / 2 / 4 column tiles, 128 with 1 / 2).  Its object is built into
// build_mfma/, beside the grouped-query decode scan's: the kernel coverage record (tests/kernel_coverage.json) is taken over
// build/ and is closed; DESIGN 6 names the test that judges these five.
#include "attention_prompt_mfma.hpp"

namespace mli {

// (the decode scan's kernels, whose header lends this file its helpers, are compiled in attention_gqa_mfma_bf16.hip alone)
#define MLI_GQA_MFMA_EXTERN(HD, NT)                                                                                              \
    extern template __global__ void gqa_mfma_scan_kernel<HD, NT>(const float*, const void* const*, const int*, float*, float2*, \
                                                                 float*, int, int, int, int, int, int, int, unsigned*, int)
MLI_GQA_MFMA_EXTERN(64, false);
MLI_GQA_MFMA_EXTERN(64, true);
MLI_GQA_MFMA_EXTERN(128, false);
MLI_GQA_MFMA_EXTERN(128, true);
#undef MLI_GQA_MFMA_EXTERN

// Every refusal, then the launch.  n_seg == 0: nothing to do.  compose.hip calls it as launch 2 of the prompt log-probabilities.
int launch_prompt_mfma_scan_elem(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                 const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q, int B,
                                 int S, int D, int H, int Hkv, int window, int n_sink, int elem, hipStream_t st) {
    if (n_seg < 0 || window < 0 || n_sink != 0 || !prompt_mfma_shape_ok(B, S, D, H, Hkv, elem)) return MLI_ERR_BAD_ARG;
    if (n_seg == 0) return 0;
    if (max_count < 1 || max_count > S || n_q < 1) return MLI_ERR_BAD_ARG;
    if (!prompt_mfma_grid_ok(n_seg, Hkv, max_count, prompt_mfma_tq(D / H, H / Hkv))) return MLI_ERR_BAD_ARG;
    if (q == nullptr || page_table == nullptr || seg_row == nullptr || seg_first == nullptr || seg_count == nullptr ||
        seg_offset == nullptr || out == nullptr)
        return MLI_ERR_BAD_ARG;
    // a window that covers the sequence is none (lean_scan_kind's hand-off)
    const int w = window < S ? window : 0;
    return launch_prompt_mfma_scan(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count, n_q, B, S, D,
                                   H, Hkv, w, st);
}

}  // namespace mli

extern "C" {

int mli_prompt_scan_mfma_shape_supported(int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int elem) {
    return mli::prompt_mfma_shape_ok(n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, elem) ? 1 : 0;
}

int mli_prompt_scan_mfma_tq(int emb_dim, int n_heads, int n_kv_heads) {
    // (the rule's limits on n_batch and n_sequence do not shape the kernel: one row of one page stands for them)
    if (!mli::prompt_mfma_shape_ok(1, mli::kPlanPage, emb_dim, n_heads, n_kv_heads, MLI_ELEM_BF16)) return MLI_ERR_BAD_ARG;
    return mli::prompt_mfma_tq(emb_dim / n_heads, n_heads / n_kv_heads);
}

int mli_prompt_scan_paged_mfma(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                               const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                               int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int window, int n_sink,
                               int elem, void* stream) {
    return mli::launch_prompt_mfma_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count, n_q,
                                             n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, elem,
                                             mli::as_stream(stream));
}

}  // extern "C"
