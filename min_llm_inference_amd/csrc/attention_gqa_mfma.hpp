// EXTENSION: the grouped-query paged decode scan on matrix instructions (bf16 pages, lean form, chunked grid, in-kernel merge).
//
// Unit of work: one (row b, K/V head j, item c).  The g = n_heads / n_kv_heads query heads j * g .. j * g + g - 1 share every K
// and V byte the workgroup loads, so the bytes AND the load instructions fall by g, and the work is split by K/V head: a row
// may be as wide as it likes (emb_dim to 8192), only head_dim (64 / 128) and g (1 .. 8) shape the kernel.  (b, j) is the
// VIRTUAL ROW vb = b * n_kv_heads + j of the launch plan (scan_plan.hpp): g * hd wide, g heads of statistics.  q and the
// output of virtual row vb are the contiguous g * hd floats at vb * g * hd, so the item sizes, the "full items + one remainder
// grid row" grid, the workspace (arrival counters | (m, l) per (virtual row, item, head) | partial rows), row_arrive and the
// last arriver's per-head merge are the multi-head scan's (heads_item_body.hpp), restated here over the virtual row.
//
// A wave owns whole pages.  Per page (16 tokens) and wave:
//   scores^T [16 tokens x 16 heads] = K [16 x hd] . q^T [hd x 16]   on v_mfma_f32_16x16x32_bf16, hd / 32 instructions per part
//     A = K: lane l holds 8 consecutive hd elements of token l % 16 -- K goes from global memory into the A registers with
//       16-byte loads, no LDS.  The 4 lanes of a token (l / 16 = 0 .. 3) read its head row as contiguous runs of hd / 4
//       elements, one 16-byte unit per instruction: instruction i contracts over hd indices (l / 16) * hd / 4 + 8 i + e.
//     B = q^T with the same permutation: lane l holds those elements of query head l % 16 (zeros from head g on).
//     C: lane l holds head l % 16, tokens 4 (l / 16) .. + 3.  Tokens are the M rows, so a NaN in the K row of a dead slot
//       reaches that slot's scores only; the mask drops them AFTER the score, by select.
//   The per-head page maximum and sum are 4 values per lane and two exchanges across the four 16-lane rows; the four lanes
//   of a head end with bit-identical (m, l) (a + b == b + a).
//   out [16 heads x hd] += P [16 x 16 tokens] . V [16 x hd]          on v_mfma_f32_16x16x16_bf16, hd / 16 instructions per part
//     A = P: lane l needs head l % 16, tokens 4 (l / 16) .. + 3 -- exactly what the C tile of the scores left in the lane: the
//       probabilities never cross lanes.  (This is why the scores are computed transposed.)
//     B = V: lane l needs V[tokens 4 (l / 16) .. + 3][column l % 16 of the tile]: the contraction index is the slow index in
//       memory, so V goes through LDS -- written as loaded (16-byte units, rows padded by 16 bytes so that the four 16-lane
//       rows of a read fall into different banks), read back with plain 2-byte reads.  A dead slot's V row is written as
//       zeros: unwritten page memory never reaches a product.
//     C: lane l holds output column l % 16 of the tile for heads 4 (l / 16) .. + 3.
//
// fp32 accuracy from bf16 operands.  q (once per item) and the page's probabilities are split into THREE bf16 parts by
// truncation, x = hi + mid + lo exactly (8 + 8 + 8 significand bits); K and V are bf16, so every product is exact in the fp32
// accumulator.  The parts are not stacked as further M rows: they are further steps of the contraction -- the same accumulator
// takes lo, mid, hi in turn (smallest first), which needs no row sum afterwards and lets one 16-row tile hold every g <= 8.
// Two parts leave a relative error of 2^-16 in every factor, 16 times the floor of the project's tolerance (16 * 2^-24):
// tests/test_gqa_mfma_scan_gpu.py shows on the CPU that fewer parts miss the bound.
//
//   grid = (B * n_kv_heads, items of the span + 1), virtual rows fast, 256 threads; one launch, no combine kernel
#pragma once

#include "heads_item_body.hpp"
#include "scan_launch.hpp"

namespace mli {

typedef __bf16 mf_bf16x8 __attribute__((ext_vector_type(8)));
typedef short mf_s16x4 __attribute__((ext_vector_type(4)));
typedef float mf_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t mf_u32x2 __attribute__((ext_vector_type(2)));

constexpr int kMfmaParts = 3;
constexpr int kMfmaMaxGroup = MLI_GQA_MFMA_MAX_GROUP;   // heads a statistics row of a wave holds

// x = part[2] + part[1] + part[0] exactly, each part a bf16 in the high half of its word (truncation: the residual of a
// truncated value keeps its sign and has 8 significand bits fewer)
__device__ __forceinline__ void mfma_split3(float x, uint32_t (&part)[kMfmaParts]) {
    part[2] = __float_as_uint(x) & 0xffff0000u;
    const float r1 = x - __uint_as_float(part[2]);
    part[1] = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(part[1]);
    part[0] = __float_as_uint(r2) & 0xffff0000u;
}
// two bf16 (high halves) -> one word, `first` in the low half (the lower element index)
__device__ __forceinline__ uint32_t mfma_pack(uint32_t first, uint32_t second) { return (first >> 16) | second; }

// LDS of a workgroup: page pointers of the item (rounded to 16 bytes) | max(the waves' V tiles + parked rows + (m, l), the
// row's (item, head) statistics during the merge).  Host and device compile this text.  tile_elem_bytes: 2, the bf16 V tile
// (bf16 and fp8 pages), or 4, the fp32 one.
constexpr size_t gqa_mfma_vtile_bytes(int hd, int tile_elem_bytes = 2) { return (size_t)16 * (hd * tile_elem_bytes + 16); }
constexpr size_t gqa_mfma_ptr_bytes(int ct) { return (((size_t)(ct / kPlanPage) * 8) + 15) & ~(size_t)15; }
constexpr size_t gqa_mfma_work_bytes(int hd, int g, int tile_elem_bytes = 2) {
    return kPlanWaves * (gqa_mfma_vtile_bytes(hd, tile_elem_bytes) + (size_t)g * hd * sizeof(float) + kMfmaMaxGroup * 8);
}

// four e4m3 bytes of a page word -> four bf16 in two words, exactly (every e4m3 value is a bf16 value: 3 significand bits, and
// the exponent range lies inside bf16's); element order kept.  ElemFP8's decode (scan_common.hpp) and the high-half pack.
__device__ __forceinline__ mf_u32x2 mfma_fp8x4_to_bf16x4(uint32_t w) {
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
    return mf_u32x2{mfma_pack(__float_as_uint(lo.x), __float_as_uint(lo.y) & 0xffff0000u),
                    mfma_pack(__float_as_uint(hi.x), __float_as_uint(hi.y) & 0xffff0000u)};
}
// 16 e4m3 bytes (one 16-byte load) -> 16 bf16: elements 0 .. 7 and 8 .. 15
__device__ __forceinline__ void mfma_fp8x16_to_bf16(const fu_u32x4& r, fu_u32x4& first, fu_u32x4& second) {
    const mf_u32x2 a = mfma_fp8x4_to_bf16x4(r.x), b = mfma_fp8x4_to_bf16x4(r.y);
    const mf_u32x2 c = mfma_fp8x4_to_bf16x4(r.z), d = mfma_fp8x4_to_bf16x4(r.w);
    first = fu_u32x4{a.x, a.y, b.x, b.y};
    second = fu_u32x4{c.x, c.y, d.x, d.y};
}

// vb = b * Hkv + j; g = query heads per K/V head; window = 0: none, else 1 <= window < S (mli_decode_scan_paged_gqa's
// semantics: the row attends slots [max(0, L - window), L), is taken from its first live page on, and that page's slots below
// the window are masked).  ml: [B * Hkv][nchunk_max][g]; partial: [B * Hkv][nchunk_max][g * HD].
// FP8: the pages hold e4m3 bytes (attention_gqa_mfma_fp8.hip has the account of that data path); everything from the score
// instructions on is the same text.
template <int HD, bool NT, bool FP8 = false>
__device__ __forceinline__ void gqa_mfma_item(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int Hkv, int g, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int vb, int c, bool first_grid_row, unsigned char* smem_raw, int window) {
    static_assert(HD == 64 || HD == 128, "head_dim 64 or 128");
    constexpr int NM = HD / 32;             // score instructions per part = 16-byte K loads = 16-byte V loads of a lane
    constexpr int EB = FP8 ? 1 : 2;         // bytes of a page element
    constexpr int NL = NM * EB / 2;         // ... of which fp8 pages need half: a 16-byte K load feeds two score instructions
    constexpr int NDT = HD / 16;            // 16-column tiles of the output
    constexpr int UPT = HD * EB / 16;       // 16-byte units of a token's V head row
    constexpr int TPI = kWave / UPT;        // tokens one V load instruction covers
    constexpr int VSTRIDE = HD * 2 + 16;    // bytes of a token row of the V tile
    constexpr int hd_shift = HD == 128 ? 7 : 6;
    const int Dg = g * HD;                  // the virtual row's width
    const int b = vb / Hkv, j = vb - b * Hkv;

    const void** ptr_sh = reinterpret_cast<const void**>(smem_raw);
    unsigned char* work = smem_raw + gqa_mfma_ptr_bytes(ct);
    unsigned char* vt_all = work;                                                                     // [waves][16][VSTRIDE]
    float* red = reinterpret_cast<float*>(work + kFuWaves * gqa_mfma_vtile_bytes(HD));                // [waves][Dg]
    float2* wave_ml = reinterpret_cast<float2*>(red + kFuWaves * Dg);                                 // [waves][kMfmaMaxGroup]
    __shared__ int last_sh;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int n16 = lane & 15;   // scores: the lane's head; K: its token; output: its column of a tile
    const int kg = lane >> 4;    // the 16-lane row: tokens 4 kg .. + 3 of the C tiles, run kg of a K head row
    const int W = S / kPage;

    const int L_row = min(lengths[b], S);
    const int lo = window > 0 ? max(0, L_row - window) : 0;   // first slot the row attends
    const int p0 = lo / kPage;                                // ... and the page it lies in
    const int L = L_row - p0 * kPage;                         // the row from that page on
    if (L <= 0) {
        // no workgroup arrives for an empty row: its zero result is written here, once
        if (first_grid_row)
            for (int i = threadIdx.x; i < Dg; i += kFuThreads) out[(int64_t)vb * Dg + i] = 0.f;
        return;
    }
    // items of a row: grid rows 0 .. nchunk-1 run the full chunks, grid row nchunk every row's remainder (fused_scan_item)
    int s0 = c * ct, s1 = min(s0 + ct, L);
    if (!direct) {
        const int nf = L / ct;
        if (c < nchunk_max) {
            if (c >= nf) return;
        } else {
            s0 = nf * ct;
            if (s0 >= L) return;
            s1 = L;
            c = nf;
        }
    }
    const int ntok = s1 - s0;
    const int npages = (ntok + kPage - 1) / kPage;   // <= ct / 16 and p0 + s0 / 16 + npages <= W
    for (int i = threadIdx.x; i < npages; i += kFuThreads) ptr_sh[i] = page_table[(int64_t)b * W + p0 + s0 / kPage + i];
    __syncthreads();

    // ---- q^T, three parts, in the B layout of the score instructions: once per item that has work ----
    fu_u32x4 qp[kMfmaParts][NM];
    {
        const float* qrow = q + (int64_t)vb * Dg + n16 * HD + kg * (HD / 4);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            uint32_t part[8][kMfmaParts];
#pragma unroll
            for (int e = 0; e < 8; ++e) mfma_split3(n16 < g ? qrow[8 * i + e] : 0.f, part[e]);
#pragma unroll
            for (int p = 0; p < kMfmaParts; ++p) {
                qp[p][i].x = mfma_pack(part[0][p], part[1][p]);
                qp[p][i].y = mfma_pack(part[2][p], part[3][p]);
                qp[p][i].z = mfma_pack(part[4][p], part[5][p]);
                qp[p][i].w = mfma_pack(part[6][p], part[7][p]);
            }
        }
    }

    const float scale = sqrtf((float)HD);
    const float inv_scale = 1.f / scale;
    const int row_bytes = 3 * D * EB;                // one token slot: x | K | V
    const int block_bytes = kPage * row_bytes;
    // K: token n16, run kg of K/V head j, one 16-byte unit per instruction.  V: TPI tokens per instruction, a head row coalesced
    const unsigned koff = (unsigned)(n16 * row_bytes + (D + j * HD + kg * (HD / 4)) * EB);
    const int vtok = lane / UPT, vunit = lane % UPT;
    const unsigned voff = (unsigned)(vtok * row_bytes + (2 * D + j * HD) * EB + vunit * 16);
    unsigned char* vt = vt_all + wave * gqa_mfma_vtile_bytes(HD);

    auto load_page = [&](int pi, fu_u32x4 (&kr)[NL], fu_u32x4 (&vr)[NL]) {
        const char* pg = reinterpret_cast<const char*>(wave_uniform(reinterpret_cast<const float*>(ptr_sh[pi])));
        // a null page gets an empty range: its loads return zeros; every offset below lies inside the page block
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(pg), 0, pg != nullptr ? block_bytes : 0, 0x00020000);
#pragma unroll
        for (int i = 0; i < NL; ++i) kr[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, koff, i * 16, NT ? 2 : 0);
#pragma unroll
        for (int i = 0; i < NL; ++i) vr[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, i * TPI * row_bytes, NT ? 2 : 0);
    };

    float run_m = -INFINITY, run_l = 0.f;   // of head n16, the same bits in the head's four lanes
    mf_f32x4 acc[NDT];                      // heads 4 kg .. + 3, column n16 of tile dt
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) acc[dt] = mf_f32x4{0.f, 0.f, 0.f, 0.f};

    fu_u32x4 kc[NL], vc[NL], kn[NL], vn[NL];   // the page being consumed and the wave's next one, in flight meanwhile
    if (wave < npages) load_page(wave, kc, vc);
    for (int pi = wave; pi < npages; pi += kFuWaves) {
        const bool has_next = pi + kFuWaves < npages;   // wave-uniform
        if (has_next) load_page(pi + kFuWaves, kn, vn);
        const int nt = min(kPage, ntok - pi * kPage);                                 // slots of this page inside the row (>= 1)
        const int nlo = (window > 0 && pi == 0 && s0 == 0) ? lo - p0 * kPage : 0;     // slots below the window
        auto live = [&](int t) { return t < nt && t >= nlo; };

        // ---- V tile -> LDS as loaded (fp8: decoded to the same bf16 tile, 32 bytes a unit), dead slots as zeros ----
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int t = i * TPI + vtok;
            const fu_u32x4 v = live(t) ? vc[i] : fu_u32x4{0u, 0u, 0u, 0u};
            if constexpr (FP8) {
                fu_u32x4 v0, v1;
                mfma_fp8x16_to_bf16(v, v0, v1);
                *reinterpret_cast<fu_u32x4*>(vt + t * VSTRIDE + vunit * 32) = v0;
                *reinterpret_cast<fu_u32x4*>(vt + t * VSTRIDE + vunit * 32 + 16) = v1;
            } else {
                *reinterpret_cast<fu_u32x4*>(vt + t * VSTRIDE + vunit * 16) = v;
            }
        }
        __builtin_amdgcn_wave_barrier();   // other lanes of the wave read the tile back below: no LDS access moves across

        // ---- scores^T: lo, mid, hi parts of q into one accumulator ----
        // (fp8: load i of the run decodes into the A fragments of instructions 2 i and 2 i + 1 -- elements 8 i' .. 8 i' + 7 of
        // the run for instruction i', the bf16 order, so q's B fragments above serve both)
        fu_u32x4 kf[NM];
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            if constexpr (FP8) mfma_fp8x16_to_bf16(kc[i], kf[2 * i], kf[2 * i + 1]);
            else kf[i] = kc[i];
        }
        mf_f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int p = 0; p < kMfmaParts; ++p)
#pragma unroll
            for (int i = 0; i < NM; ++i)
                sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mf_bf16x8, kf[i]),
                                                             __builtin_bit_cast(mf_bf16x8, qp[p][i]), sc, 0, 0, 0);

        // ---- online softmax of head n16 over the page: 4 tokens here, the rest in the other three 16-lane rows ----
        float s[4];
        float pm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s[r] = div_by(sc[r], scale, inv_scale);
            pm = live(4 * kg + r) ? fmaxf(pm, s[r]) : pm;
        }
        pm = fmaxf(pm, __shfl_xor(pm, 16, kWave));
        pm = fmaxf(pm, __shfl_xor(pm, 32, kWave));
        const float m_new = fmaxf(run_m, pm);
        const float alpha = run_m == -INFINITY ? 0.f : expf(run_m - m_new);
        float psum = 0.f;
        uint32_t pp[4][kMfmaParts];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pr = live(4 * kg + r) ? expf(s[r] - m_new) : 0.f;
            psum += pr;
            mfma_split3(pr, pp[r]);
        }
        psum += __shfl_xor(psum, 16, kWave);
        psum += __shfl_xor(psum, 32, kWave);
        run_l = run_l * alpha + psum;
        run_m = m_new;
        // the output tile holds heads 4 kg .. + 3: their alpha lives in lanes 4 kg .. + 3 (any 16-lane row holds head l % 16)
        float al[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) al[r] = __shfl(alpha, 4 * kg + r, kWave);
        mf_s16x4 pa[kMfmaParts];
#pragma unroll
        for (int p = 0; p < kMfmaParts; ++p)
            pa[p] = __builtin_bit_cast(mf_s16x4, mf_u32x2{mfma_pack(pp[0][p], pp[1][p]), mfma_pack(pp[2][p], pp[3][p])});

        // ---- out += P . V per 16-column tile, V read back transposed ----
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const unsigned short* col = reinterpret_cast<const unsigned short*>(vt + (4 * kg) * VSTRIDE + (dt * 16 + n16) * 2);
            const uint32_t v0 = col[0], v1 = col[VSTRIDE / 2], v2 = col[2 * (VSTRIDE / 2)], v3 = col[3 * (VSTRIDE / 2)];
            const mf_s16x4 vb4 = __builtin_bit_cast(mf_s16x4, mf_u32x2{v0 | (v1 << 16), v2 | (v3 << 16)});
            mf_f32x4 a = acc[dt];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] *= al[r];
#pragma unroll
            for (int p = 0; p < kMfmaParts; ++p) a = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa[p], vb4, a, 0, 0, 0);
            acc[dt] = a;
        }
        __builtin_amdgcn_wave_barrier();   // ... and the next page's tile is written only behind these reads
        if (has_next) {
#pragma unroll
            for (int i = 0; i < NL; ++i) {
                kc[i] = kn[i];
                vc[i] = vn[i];
            }
        }
    }

    // ---- the item's result per head: the waves (each owns whole pages) are merged in wave order through LDS ----
    const bool publish = !direct;
    float* o = direct ? out + (int64_t)vb * Dg : partial + ((int64_t)vb * nchunk_max + c) * Dg;
    if (lane < kMfmaMaxGroup) wave_ml[wave * kMfmaMaxGroup + lane] = make_float2(run_m, run_l);
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (4 * kg + r < g) red[wave * Dg + (4 * kg + r) * HD + dt * 16 + n16] = acc[dt][r];
    __syncthreads();
    const __amdgpu_buffer_rsrc_t orow = __builtin_amdgcn_make_buffer_rsrc(o, 0, Dg * (int)sizeof(float), 0x00020000);
    for (int i = 4 * threadIdx.x; i < Dg; i += 4 * kFuThreads) {
        const int h = i >> hd_shift;   // the four elements of a thread share a head
        float m = -INFINITY;
#pragma unroll
        for (int w = 0; w < kFuWaves; ++w) m = fmaxf(m, wave_ml[w * kMfmaMaxGroup + h].x);
        float wsc[kFuWaves];
        float l = 0.f;
#pragma unroll
        for (int w = 0; w < kFuWaves; ++w) {
            const float2 st = wave_ml[w * kMfmaMaxGroup + h];
            wsc[w] = st.x == -INFINITY ? 0.f : expf(st.x - m);
            l += st.y * wsc[w];
        }
        const float norm = direct ? 1.f / l : 1.f;
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < kFuWaves; ++w) t += red[w * Dg + i + k] * wsc[w];
            r[k] = t * norm;
        }
        if (publish) {
            // write-through (sc1) stores: another workgroup may read the row back inside this launch
            fu_u32x4 raw;
            raw.x = __float_as_uint(r[0]); raw.y = __float_as_uint(r[1]); raw.z = __float_as_uint(r[2]); raw.w = __float_as_uint(r[3]);
            __builtin_amdgcn_raw_buffer_store_b128(raw, orow, i * (int)sizeof(float), 0, 16);
            if ((i & (HD - 1)) == 0) {   // the head's first element: its (m, l) goes with it
                typedef unsigned long long __attribute__((address_space(1)))* gu64_ptr;
                const unsigned long long packed = ((unsigned long long)__float_as_uint(l) << 32) | __float_as_uint(m);
                __hip_atomic_store((gu64_ptr)(ml + ((int64_t)vb * nchunk_max + c) * g + h), packed, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);  // sc1 store
            }
        } else {
            *reinterpret_cast<float4*>(o + i) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
    if (!publish) return;

    // ---- count the arrival; the workgroup that completes the virtual row merges its items per head, in item order ----
    const int nc = (L + ct - 1) / ct;
    if (!row_arrive(arrivals + vb, nc, &last_sh)) return;
    typedef unsigned long long __attribute__((address_space(1)))* gu64_ptr;
    float2* ml_sh = reinterpret_cast<float2*>(work);   // [nc][g]; the barriers of row_arrive lie behind the last read of red
    const float2* ml_row = ml + (int64_t)vb * nchunk_max * g;
    for (int i = threadIdx.x; i < nc * g; i += kFuThreads) {
        const unsigned long long packed = __hip_atomic_load((gu64_ptr)(ml_row + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ml_sh[i] = make_float2(__uint_as_float((unsigned)packed), __uint_as_float((unsigned)(packed >> 32)));
    }
    __syncthreads();
    const float* partial_row = partial + (int64_t)vb * nchunk_max * Dg;
    float* out_row = out + (int64_t)vb * Dg;
    for (int d = 4 * threadIdx.x; d < Dg; d += 4 * kFuThreads) {
        const int h = d >> hd_shift;
        float mm = -INFINITY;
        for (int i = 0; i < nc; ++i) mm = fmaxf(mm, ml_sh[i * g + h].x);
        float ll = 0.f;
        for (int i = 0; i < nc; ++i) ll = fmaf(ml_sh[i * g + h].y, expf(ml_sh[i * g + h].x - mm), ll);
        const float inv_l = 1.f / ll;
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = 0; i0 < nc; i0 += 8) {   // up to 8 partial rows in flight
            fu_u32x4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (i0 + k < nc) {
                    const float* row_i = partial_row + (int64_t)(i0 + k) * Dg;
                    const __amdgpu_buffer_rsrc_t prow =
                        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row_i), 0, Dg * (int)sizeof(float), 0x00020000);
                    v[k] = __builtin_amdgcn_raw_buffer_load_b128(prow, d * (int)sizeof(float), 0, 16);   // sc1: never L1
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (i0 + k < nc) {
                    const float w = expf(ml_sh[(i0 + k) * g + h].x - mm);
                    r[0] = fmaf(__uint_as_float(v[k].x), w, r[0]);
                    r[1] = fmaf(__uint_as_float(v[k].y), w, r[1]);
                    r[2] = fmaf(__uint_as_float(v[k].z), w, r[2]);
                    r[3] = fmaf(__uint_as_float(v[k].w), w, r[3]);
                }
            }
        }
        *reinterpret_cast<float4*>(out_row + d) = make_float4(r[0] * inv_l, r[1] * inv_l, r[2] * inv_l, r[3] * inv_l);
    }
}

template <int HD, bool NT>
__global__ __launch_bounds__(kFuThreads, 2) void gqa_mfma_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int Hkv, int g, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // virtual rows rotated by the item index: the items of one row spread over the XCDs (fused_decode_scan_kernel)
    const int c = blockIdx.y;
    const int vb = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    gqa_mfma_item<HD, NT>(q, page_table, lengths, out, ml, partial, S, D, Hkv, g, ct, nchunk_max, direct, arrivals, vb, c,
                          c == 0, smem_raw, window);
}

// The plan is the chunked scans' (scan_plan.hpp) over B * Hkv virtual rows of g heads, g * hd wide, hd columns read; rows are
// taken in grid order.  window: 0 = none (the caller has handed a window that covers n_sequence on as none).
inline ScanPlan gqa_mfma_plan(const ScanTune& tune, int B, int S, int D, int H, int Hkv, int window, int elem_bytes = 2) {
    ScanTune t = tune;
    t.row_order = 0;
    const int hd = D / H, g = H / Hkv;
    return plan_chunked_scan(t, B * Hkv, S, window > 0 ? window_span(S, window) : S, g * hd, hd, g, elem_bytes);
}

// The page element type of a launch: its bytes (the plan's item sizing and NT rule), its launch family, its four kernels.
struct GqaMfmaBf16 {
    static constexpr int kBytes = 2;
    static constexpr int kTileBytes = 2;   // of a V tile element in LDS
    static constexpr LaunchFamily kFamily = kLfScanGqaMfma;
    template <int HD, bool NT>
    static constexpr auto kernel() { return &gqa_mfma_scan_kernel<HD, NT>; }
};

// After gqa_mfma_shape_ok (P = GqaMfmaFp8: gqa_mfma_fp8_shape_ok, GqaMfmaF32: gqa_mfma_f32_shape_ok); ws = the workspace body.
template <class P = GqaMfmaBf16>
inline int launch_gqa_mfma_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S,
                                int D, int H, int Hkv, int window, void* ws, size_t ws_bytes, hipStream_t st) {
    const int hd = D / H, g = H / Hkv;
    const ScanPlan p = gqa_mfma_plan(scan_tune(), B, S, D, H, Hkv, window, P::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return MLI_ERR_WORKSPACE;
    const size_t work = gqa_mfma_work_bytes(hd, g, P::kTileBytes), merge = heads_merge_stat_bytes(p.nchunk, g);
    const size_t smem = gqa_mfma_ptr_bytes(p.ct) + (work > merge ? work : merge);
    if (!scan_lds_fits(smem)) return MLI_ERR_BAD_ARG;   // (gqa_mfma_shape_ok keeps every accepted shape inside)
    count_launch(P::kFamily);
    const dim3 grid(B * Hkv, p.grid_y), block(kFuThreads);
    const auto go = [&](auto hdc, auto nt) {
        hipLaunchKernelGGL((P::template kernel<decltype(hdc)::value, decltype(nt)::value>()), grid, block, smem, st, q, page_table,
                           lengths, out, w.ml, w.partial, S, D, Hkv, g, p.ct, p.nchunk, p.direct, w.arrivals, window);
    };
    using std::integral_constant;
    if (hd == 128) p.nt ? go(integral_constant<int, 128>{}, std::true_type{}) : go(integral_constant<int, 128>{}, std::false_type{});
    else p.nt ? go(integral_constant<int, 64>{}, std::true_type{}) : go(integral_constant<int, 64>{}, std::false_type{});
    return launch_status();
}

}  // namespace mli
