// The grouped-query paged decode scan on matrix instructions over bf16 pages: attention_gqa_mfma.hpp has the account and the
// kernel.  Four kernels (head_dim 64 / 128, default / non-temporal K and V loads).  Its object is built into build_mfma/, not
// build/: the kernel coverage record (tests/kernel_coverage.json) is taken over build/ and judged by a list this extension
// may not edit; DESIGN 6 names the test that judges these four.
#include "attention_gqa_mfma.hpp"

namespace mli {

// compose.hip: after gqa_mfma_shape_ok, over the workspace body; window 0 = none
int launch_gqa_mfma_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                           int H, int Hkv, int window, void* ws, size_t ws_bytes, hipStream_t st) {
    return launch_gqa_mfma_scan(q, page_table, lengths, out, B, S, D, H, Hkv, window, ws, ws_bytes, st);
}

}  // namespace mli
