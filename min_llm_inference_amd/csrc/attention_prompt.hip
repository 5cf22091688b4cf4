// The causal multi-query prompt scan over fp32 pages, and the scan's entry points: attention_prompt.hpp has the kernel, the
// launcher and the account; the bf16 kernels are compiled in attention_prompt_bf16.hip.
#include <cmath>

#include "attention_prompt.hpp"

namespace mli {
template int launch_prompt_scan<ElemF32>(const float*, const void* const*, const int*, const int*, const int*, const int*, float*,
                                         int, int, int, int, int, int, int, int, int, int, int, hipStream_t);
extern template int launch_prompt_scan<ElemBF16>(const float*, const void* const*, const int*, const int*, const int*, const int*,
                                                 float*, int, int, int, int, int, int, int, int, int, int, int, hipStream_t);
template int launch_prompt_softcap_scan<ElemF32>(const float*, const void* const*, const int*, const int*, const int*, const int*,
                                                 float*, int, int, int, int, int, int, int, int, int, int, int, float, hipStream_t);
extern template int launch_prompt_softcap_scan<ElemBF16>(const float*, const void* const*, const int*, const int*, const int*,
                                                         const int*, float*, int, int, int, int, int, int, int, int, int, int, int,
                                                         float, hipStream_t);
template int launch_prompt_sink_logits_scan<ElemF32>(const float*, const void* const*, const int*, const int*, const int*,
                                                     const int*, float*, int, int, int, int, int, int, int, int, int, int, int,
                                                     const float*, hipStream_t);
extern template int launch_prompt_sink_logits_scan<ElemBF16>(const float*, const void* const*, const int*, const int*, const int*,
                                                             const int*, float*, int, int, int, int, int, int, int, int, int, int,
                                                             int, const float*, hipStream_t);

// The scan for the compositions (compose.hip) and the entry points: every refusal, then the launch.  n_seg == 0: nothing to do.
// capped: the scan with logit soft-capping (attention_softcap.hpp) -- two heads at least and a finite cap > 0, or a bad argument.
// sunk: the scan with a learned sink logit per query head (attention_sink_logits.hpp) -- two heads at least and a non-null
// sink_logits (n_heads floats in device memory), or a bad argument.
static int prompt_scan_elem(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                            const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q, int B,
                            int S, int D, int H, int Hkv, int window, int n_sink, int elem, bool capped, float cap,
                            hipStream_t st, bool sunk = false, const float* sink_logits = nullptr) {
    if (capped && (H < 2 || !(cap > 0.f) || !std::isfinite(cap))) return MLI_ERR_BAD_ARG;
    if (sunk && (H < 2 || sink_logits == nullptr)) return MLI_ERR_BAD_ARG;
    if (n_seg < 0 || window < 0 || n_sink < 0 || !prompt_scan_shape_ok(B, S, D, H, Hkv, elem)) return MLI_ERR_BAD_ARG;
    if (n_seg == 0) return 0;
    if (max_count < 1 || max_count > S || n_q < 1) return MLI_ERR_BAD_ARG;
    const int epl = elem == MLI_ELEM_BF16 ? 8 : 4;
    if (!prompt_scan_grid_ok(n_seg, max_count, prompt_scan_tq(epl, plan_ceil_div(D / epl, kPlanWave), H > 1))) return MLI_ERR_BAD_ARG;
    if (q == nullptr || page_table == nullptr || seg_row == nullptr || seg_first == nullptr || seg_count == nullptr ||
        seg_offset == nullptr || out == nullptr)
        return MLI_ERR_BAD_ARG;
    // no window, or sinks and window that leave no query a gap: the plain causal mask (lean_scan_kind's hand-offs)
    const ScanKind kind = lean_scan_kind(S, window, n_sink);
    const int w = kind == kScanPlain ? 0 : window, k = kind == kScanSinks ? n_sink : 0;
    const int lg = H > 1 ? heads_lanes_log2(B, S, D, H, elem) : 0;
    if (sunk) {
        if (elem == MLI_ELEM_BF16)
            return launch_prompt_sink_logits_scan<ElemBF16>(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg,
                                                            max_count, n_q, B, S, D, H, Hkv, lg, w, k, sink_logits, st);
        return launch_prompt_sink_logits_scan<ElemF32>(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg,
                                                       max_count, n_q, B, S, D, H, Hkv, lg, w, k, sink_logits, st);
    }
    if (capped) {
        if (elem == MLI_ELEM_BF16)
            return launch_prompt_softcap_scan<ElemBF16>(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg,
                                                        max_count, n_q, B, S, D, H, Hkv, lg, w, k, cap, st);
        return launch_prompt_softcap_scan<ElemF32>(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count,
                                                   n_q, B, S, D, H, Hkv, lg, w, k, cap, st);
    }
    if (elem == MLI_ELEM_BF16)
        return launch_prompt_scan<ElemBF16>(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count, n_q,
                                            B, S, D, H, Hkv, lg, w, k, st);
    return launch_prompt_scan<ElemF32>(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count, n_q, B, S,
                                       D, H, Hkv, lg, w, k, st);
}
int launch_prompt_scan_elem(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                            const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q, int B,
                            int S, int D, int H, int Hkv, int window, int n_sink, int elem, hipStream_t st) {
    return prompt_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count, n_q, B, S, D, H, Hkv,
                            window, n_sink, elem, false, 0.f, st);
}
int launch_prompt_softcap_scan_elem(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                    const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                                    int B, int S, int D, int H, int Hkv, int window, int n_sink, float cap, int elem,
                                    hipStream_t st) {
    return prompt_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count, n_q, B, S, D, H, Hkv,
                            window, n_sink, elem, true, cap, st);
}
int launch_prompt_sink_logits_scan_elem(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                        const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                                        int B, int S, int D, int H, int Hkv, int window, int n_sink, const float* sink_logits,
                                        int elem, hipStream_t st) {
    return prompt_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count, n_q, B, S, D, H, Hkv,
                            window, n_sink, elem, false, 0.f, st, true, sink_logits);
}
}  // namespace mli

extern "C" {

int mli_prompt_scan_tq(int emb_dim, int n_heads, int elem) {
    if ((elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) || emb_dim <= 0 || n_heads < 1) return MLI_ERR_BAD_ARG;
    const int epl = elem == MLI_ELEM_BF16 ? 8 : 4;
    const int nj = mli::plan_ceil_div(emb_dim / epl, mli::kPlanWave);
    if (emb_dim % epl != 0 || nj > 2) return MLI_ERR_BAD_ARG;
    return mli::prompt_scan_tq(epl, nj, n_heads > 1);
}

int mli_prompt_scan_paged_softcap(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                  const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                                  int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int window, int n_sink,
                                  float cap, int elem, void* stream) {
    return mli::launch_prompt_softcap_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count,
                                                n_q, n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, cap, elem,
                                                mli::as_stream(stream));
}

int mli_prompt_scan_paged_sink_logits(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                      const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                                      int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int window,
                                      int n_sink, const float* sink_logits, int elem, void* stream) {
    return mli::launch_prompt_sink_logits_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg,
                                                    max_count, n_q, n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window,
                                                    n_sink, sink_logits, elem, mli::as_stream(stream));
}

int mli_prompt_scan_paged(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                          const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                          int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int window, int n_sink, int elem,
                          void* stream) {
    return mli::launch_prompt_scan_elem(q, page_table, seg_row, seg_first, seg_count, seg_offset, out, n_seg, max_count, n_q,
                                        n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, elem,
                                        mli::as_stream(stream));
}

}  // extern "C"
