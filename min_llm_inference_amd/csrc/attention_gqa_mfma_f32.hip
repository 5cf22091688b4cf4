// EXTENSION: the grouped-query paged decode scan on matrix instructions over fp32 pages.
//
// What it computes, its unit of work (row, K/V head, item), virtual rows, plan (element size 4), grid, workspace, arrival
// counters, window, null pages and dead slots are attention_gqa_mfma.hpp's, and so are the waves' merge, the publish and the
// last arriver's merge, restated below as gqa_mfma_f32_finish.  The data path is this file's own: fp32 pages go into
// v_mfma_f32_16x16x4_f32 as they are -- no split of q, none of the probabilities, one product per score in place of the nine
// a three-part split of both operands would need.
//
// A wave owns whole pages; its next page is in flight while one is consumed.  Per page (16 tokens) and wave:
//   scores^T [16 tokens x 16 heads] = K [16 x hd] . q^T [hd x 16]      hd / 4 instructions
//     A = K: lane l owns run l / 16 (hd / 4 floats) of token l % 16's head row, fetched from global memory with hd / 16
//       16-byte buffer loads, no LDS.  Load i gives the A operands of instructions (i, 0 .. 3): instruction (i, e) contracts
//       over the hd indices (l / 16) * hd / 4 + 4 i + e, one per 16-lane row.
//     B = q^T with the same permutation: lane l holds those hd / 4 floats of query head l % 16, zeros from head g on; read
//       once per item, by workgroups that have an item to run.
//     C: lane l holds head l % 16, tokens 4 (l / 16) .. + 3 -- the bf16 kernel's tile, so the online softmax (two exchanges
//       across the 16-lane rows per head, bit-identical (m, l) in a head's four lanes) is that kernel's text.  A NaN in the K
//       row of a dead slot reaches that slot's scores only; the mask drops them after the score, by select.
//   out [16 heads x hd] += P [16 x 16 tokens] . V [16 x hd]            hd / 16 column tiles x 4 contraction steps
//     A, step r = the lane's own probability of token 4 (l / 16) + r: the probabilities never cross lanes.
//     B, step r = V[token 4 (l / 16) + r][column l % 16 of the tile], from the wave's fp32 LDS tile [16][hd * 4 + 16 bytes],
//       written as loaded in 16-byte units (a dead slot's row as zeros) and read with 4-byte reads.  The pad: the four
//       16-lane rows of a read are 4 token rows = 4 * (hd * 4 + 16) bytes = hd * 4 + 16 words apart, which is 16 modulo 64
//       (and modulo 32), so row k of the read starts at bank 16 k and the 64 lanes fall on 64 different banks.
//     C: lane l holds output column l % 16 of the tile for heads 4 (l / 16) .. + 3.
//
// Registers.  A page is hd / 16 K loads and hd / 16 V loads of 4 registers a lane: 64 VGPRs at head_dim 128, 128 with the
// next page, beside 32 accumulators and 32 of q.  V leaves for LDS as the first thing an iteration does, so at the score
// instructions the lane holds K of this page and K, V of the next.  No scratch (DESIGN 3.1p has the table).
//
// Four kernels (head_dim 64 / 128, default / non-temporal loads).  Built into build_mfma/ (Makefile), outside the kernel
// coverage record; DESIGN 6 names the test that judges these four.
#include "attention_gqa_mfma.hpp"

namespace mli {

// The end of an item: the waves' merge, the publish and the last arriver's merge -- gqa_mfma_item's text from "the item's result
// per head" on, restated (sharing it as a function changed the register allocation of the eight bf16 / fp8 kernels, DESIGN
// 3.1p).  acc = heads 4 kg .. + 3, column n16 of tile dt; (run_m, run_l) of head n16; red: [waves][g * HD]; wave_ml:
// [waves][kMfmaMaxGroup]; work: the LDS behind the page pointers, free for the row's statistics once the waves are merged.
template <int HD>
__device__ __forceinline__ void gqa_mfma_f32_finish(
    const mf_f32x4 (&acc)[HD / 16], float run_m, float run_l, float* red, float2* wave_ml, unsigned char* work,
    float* __restrict__ out, float2* ml, float* partial, int g, int ct, int nchunk_max, int direct, unsigned* arrivals, int vb,
    int c, int L) {
    constexpr int NDT = HD / 16;
    constexpr int hd_shift = HD == 128 ? 7 : 6;
    const int Dg = g * HD;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, n16 = lane & 15, kg = lane >> 4;
    __shared__ int last_sh;

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
__device__ __forceinline__ void gqa_mfma_f32_item(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int Hkv, int g, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int vb, int c, bool first_grid_row, unsigned char* smem_raw, int window) {
    static_assert(HD == 64 || HD == 128, "head_dim 64 or 128");
    constexpr int NL = HD / 16;             // 16-byte K loads of a lane and page = its 16-byte V loads
    constexpr int NDT = HD / 16;            // 16-column tiles of the output
    constexpr int UPT = HD / 4;             // 16-byte units of a token's V head row
    constexpr int TPI = kWave / UPT;        // tokens one V load instruction covers
    constexpr int VSTRIDE = HD * 4 + 16;    // bytes of a token row of the V tile
    static_assert((size_t)16 * VSTRIDE == gqa_mfma_vtile_bytes(HD, 4), "the host sizes the tile");
    const int Dg = g * HD;                  // the virtual row's width
    const int b = vb / Hkv, j = vb - b * Hkv;

    const void** ptr_sh = reinterpret_cast<const void**>(smem_raw);
    unsigned char* work = smem_raw + gqa_mfma_ptr_bytes(ct);
    float* red = reinterpret_cast<float*>(work + kFuWaves * gqa_mfma_vtile_bytes(HD, 4));             // [waves][Dg]
    float2* wave_ml = reinterpret_cast<float2*>(red + kFuWaves * Dg);                                 // [waves][kMfmaMaxGroup]

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
    // items of a row: grid rows 0 .. nchunk-1 run the full chunks, grid row nchunk every row's remainder (gqa_mfma_item)
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

    // ---- q^T in the B layout of the score instructions, as it is: once per item that has work ----
    mf_f32x4 qb[NL];
    {
        const mf_f32x4* qrow = reinterpret_cast<const mf_f32x4*>(q + (int64_t)vb * Dg + n16 * HD + kg * (HD / 4));
#pragma unroll
        for (int i = 0; i < NL; ++i) qb[i] = n16 < g ? qrow[i] : mf_f32x4{0.f, 0.f, 0.f, 0.f};
    }

    const float scale = sqrtf((float)HD);
    const float inv_scale = 1.f / scale;
    const int row_bytes = 3 * D * 4;                 // one token slot: x | K | V
    const int block_bytes = kPage * row_bytes;
    // K: token n16, run kg of K/V head j, one 16-byte unit per load.  V: TPI tokens per instruction, a head row coalesced
    const unsigned koff = (unsigned)(n16 * row_bytes + (D + j * HD + kg * (HD / 4)) * 4);
    const int vtok = lane / UPT, vunit = lane % UPT;
    const unsigned voff = (unsigned)(vtok * row_bytes + (2 * D + j * HD) * 4 + vunit * 16);
    unsigned char* vt = work + wave * gqa_mfma_vtile_bytes(HD, 4);

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
        const int nt = min(kPage, ntok - pi * kPage);                                 // slots of this page inside the row (>= 1)
        const int nlo = (window > 0 && pi == 0 && s0 == 0) ? lo - p0 * kPage : 0;     // slots below the window
        auto live = [&](int t) { return t < nt && t >= nlo; };

        // ---- V tile -> LDS as loaded, dead slots as zeros; its registers are free before the next page's loads are issued ----
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const int t = i * TPI + vtok;
            *reinterpret_cast<fu_u32x4*>(vt + t * VSTRIDE + vunit * 16) = live(t) ? vc[i] : fu_u32x4{0u, 0u, 0u, 0u};
        }
        if (has_next) load_page(pi + kFuWaves, kn, vn);
        __builtin_amdgcn_wave_barrier();   // other lanes of the wave read the tile back below: no LDS access moves across

        // ---- scores^T: load i feeds instructions (i, 0 .. 3) ----
        mf_f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NL; ++i) {
            const mf_f32x4 ka = __builtin_bit_cast(mf_f32x4, kc[i]);
#pragma unroll
            for (int e = 0; e < 4; ++e) sc = __builtin_amdgcn_mfma_f32_16x16x4f32(ka[e], qb[i][e], sc, 0, 0, 0);
        }

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
        float pr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            pr[r] = live(4 * kg + r) ? expf(s[r] - m_new) : 0.f;
            psum += pr[r];
        }
        psum += __shfl_xor(psum, 16, kWave);
        psum += __shfl_xor(psum, 32, kWave);
        run_l = run_l * alpha + psum;
        run_m = m_new;
        // the output tile holds heads 4 kg .. + 3: their alpha lives in lanes 4 kg .. + 3 (any 16-lane row holds head l % 16)
        float al[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) al[r] = __shfl(alpha, 4 * kg + r, kWave);

        // ---- out += P . V per 16-column tile, V read back transposed: step r contracts token 4 kg + r ----
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const float* col = reinterpret_cast<const float*>(vt + (4 * kg) * VSTRIDE + (dt * 16 + n16) * 4);
            mf_f32x4 a = acc[dt];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] *= al[r];
#pragma unroll
            for (int r = 0; r < 4; ++r) a = __builtin_amdgcn_mfma_f32_16x16x4f32(pr[r], col[r * (VSTRIDE / 4)], a, 0, 0, 0);
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

    gqa_mfma_f32_finish<HD>(acc, run_m, run_l, red, wave_ml, work, out, ml, partial, g, ct, nchunk_max, direct, arrivals, vb, c, L);
}

template <int HD, bool NT>
__global__ __launch_bounds__(kFuThreads, 2) void gqa_mfma_f32_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int Hkv, int g, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int window) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // virtual rows rotated by the item index, as gqa_mfma_scan_kernel
    const int c = blockIdx.y;
    const int vb = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    gqa_mfma_f32_item<HD, NT>(q, page_table, lengths, out, ml, partial, S, D, Hkv, g, ct, nchunk_max, direct, arrivals, vb, c,
                              c == 0, smem_raw, window);
}

struct GqaMfmaF32 {
    static constexpr int kBytes = 4;
    static constexpr int kTileBytes = 4;
    static constexpr LaunchFamily kFamily = kLfScanGqaMfmaF32;
    template <int HD, bool NT>
    static constexpr auto kernel() { return &gqa_mfma_f32_scan_kernel<HD, NT>; }
};

// compose.hip: after gqa_mfma_f32_shape_ok, over the workspace body; window 0 = none
int launch_gqa_mfma_f32_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                               int H, int Hkv, int window, void* ws, size_t ws_bytes, hipStream_t st) {
    return launch_gqa_mfma_scan<GqaMfmaF32>(q, page_table, lengths, out, B, S, D, H, Hkv, window, ws, ws_bytes, st);
}

}  // namespace mli
