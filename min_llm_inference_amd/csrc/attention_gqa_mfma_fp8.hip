// EXTENSION: the grouped-query paged decode scan on matrix instructions over fp8 (OCP e4m3) pages.
//
// What it computes, its unit of work (row, K/V head, item), plan, workspace, arrival counters, merge, window, null pages and
// dead slots are attention_gqa_mfma.hpp's: gqa_mfma_item<HD, NT, FP8 = true> is that text, and this account covers what the
// page type changes -- the way from global memory to the operands of the two matrix instructions.  A slot row is x | K | V,
// 3 * D bytes; every e4m3 value is a bf16 value, so the decode is exact and the three-part bf16 split of q and of the
// probabilities gives fp32 accuracy as it does over bf16 pages.
//
// K.  Lane l owns run l / 16 of token l % 16's head row: hd / 4 consecutive elements = hd / 4 BYTES, so ONE 16-byte buffer
//   load per page at head_dim 64 and two at 128 (bf16 pages: two and four).  A load's 16 bytes are decoded in registers
//   (v_cvt_pk_f32_fp8 on each half of each word, the two results packed by their high halves) into TWO A fragments of
//   v_mfma_f32_16x16x32_bf16: bytes 0 .. 7 and 8 .. 15.  Instruction i of a lane therefore contracts elements 8 i .. 8 i + 7 of
//   its run -- the bf16 kernel's contraction order exactly, so q's B fragments are built by the same text and, on a pool that
//   holds the same values, the two kernels accumulate the same products in the same order: bit-identical results
//   (tests/test_gqa_mfma_fp8_scan_gpu.py holds them to that).  The decoded fragments live for the page's three parts only; the
//   registers in flight (this page and the next, raw) are half the bf16 kernel's, and the decoded fragments take their place.
// V.  One 16-byte load covers a whole page at head_dim 64 (4 units a token x 16 tokens), two at 128.  LDS layout (a): the
//   bytes are decoded BEFORE the LDS write, each lane writing its 16 elements as two 16-byte units into the bf16 kernel's
//   tile ([16 tokens][hd * 2 + 16 bytes]); the softmax . V phase with its 2-byte transposed reads is then shared text.  A
//   dead slot's raw bytes are replaced by zeros before the decode (0x00 decodes to +0).  Why (a): the phase after the write is
//   the one the bf16 kernel's tests and measurements already cover, and the write side costs 8 conversions and 2 LDS stores a
//   lane and page.  Layout (b) -- an fp8 tile of half the bytes, 1-byte reads, decode into the B fragment -- halves LDS bytes
//   but puts the decode (16 tiles x 4 bytes a lane) behind every read; it was not built.  DESIGN 3.1o has the measurements that
//   would call for it.
//   gfx950's packed fp8 -> bf16 conversion with a scale operand was not tried: the pair above is the decode the project's
//   other fp8 kernels are already held to.
//
// Four kernels (head_dim 64 / 128, default / non-temporal loads), launch bounds as the bf16 kernels', no scratch (DESIGN 3.1o
// has the register table).  Built into build_mfma/ (Makefile), outside the kernel coverage record; DESIGN 6 names the test that
// judges these four.
#include "attention_gqa_mfma.hpp"

namespace mli {

template <int HD, bool NT>
__global__ __launch_bounds__(kFuThreads, 2) void gqa_mfma_fp8_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int Hkv, int g, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // virtual rows rotated by the item index, as gqa_mfma_scan_kernel
    const int c = blockIdx.y;
    const int vb = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    gqa_mfma_item<HD, NT, true>(q, page_table, lengths, out, ml, partial, S, D, Hkv, g, ct, nchunk_max, direct, arrivals, vb, c,
                                c == 0, smem_raw, window);
}

struct GqaMfmaFp8 {
    static constexpr int kBytes = 1;
    static constexpr int kTileBytes = 2;
    static constexpr LaunchFamily kFamily = kLfScanGqaMfmaFp8;
    template <int HD, bool NT>
    static constexpr auto kernel() { return &gqa_mfma_fp8_scan_kernel<HD, NT>; }
};

// compose.hip: after gqa_mfma_fp8_shape_ok, over the workspace body; window 0 = none
int launch_gqa_mfma_fp8_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                               int H, int Hkv, int window, void* ws, size_t ws_bytes, hipStream_t st) {
    return launch_gqa_mfma_scan<GqaMfmaFp8>(q, page_table, lengths, out, B, S, D, H, Hkv, window, ws, ws_bytes, st);
}

}  // namespace mli
