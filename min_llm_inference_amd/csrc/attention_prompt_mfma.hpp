// EXTENSION: the causal multi-query prompt scan on matrix instructions (bf16 pages).  It computes what mli_prompt_scan_paged
// computes (attention_prompt.hpp has the semantics of segments, mask and window), with the operand layouts, the transposed
// score tile, the V tile through LDS and the exact three-part bf16 split of the grouped-query decode scan
// (attention_gqa_mfma.hpp has that account; mfma_split3 and mfma_pack are its text).
//
// Unit of work: one 256-thread workgroup per (segment, K/V head j, block of TQ consecutive queries).  The N columns of the
// matrix instructions are the TQ * g (query, head of the group) pairs, column = query * g + head, cut into NC = TQ * g / 16
// column tiles; g = n_heads / n_kv_heads is a power of two up to 8, so a tile never holds a partial group and TQ = 16 NC / g.
// TQ is at most 16 (a block then wastes less than one page on its causal skew) and NC at most prompt_mfma_max_tiles(head_dim),
// the most that compiles without scratch: 4 at head_dim 64 (TQ = 16, 16, 16, 8 for g = 1, 2, 4, 8), 2 at 128 (16, 16, 8, 4).
// A column whose query lies beyond the segment's count has zero q, attends nothing and is never written.
//
// A wave owns whole pages of the block's attended prefix: pages [lo0 / 16, t_hi / 16], lo0 the first slot the block's FIRST
// query attends, t_hi the position of its LAST one.  Pages outside are never visited and their table entries never read.
// Per page (16 tokens) and wave:
//   K: hd / 32 16-byte loads per lane, straight into the A registers, ONCE -- they serve the NC score tiles
//   scores^T [16 tokens x 16 columns] per tile on v_mfma_f32_16x16x32_bf16, q's lo, mid, hi parts into one accumulator
//     (q is split once per block and stays in registers in the B layout)
//   mask per (column's query position, token) by select after the score; online softmax per column (the four lanes of a
//     column end with the same bits); the probabilities are split into three parts where they are
//   V: written to the wave's padded LDS tile ONCE per page, a slot no query of the block attends as zeros (NaN in unwritten
//     slots never reaches a product); every 16-column fragment read back transposed once and used by the NC column tiles
//   out [16 columns x hd] += P . V per tile on v_mfma_f32_16x16x16_bf16
// There is no split along the key axis, no workspace and no arrival counter: the four waves' (m, l, O) are merged through LDS
// at the end, one column tile at a time, and written to the dense rows.
//
//   grid = n_seg * ceil(max_count / TQ) * n_kv_heads workgroups (K/V heads fast; surplus ones exit), 256 threads, static LDS
#pragma once

#include "attention_gqa_mfma.hpp"

namespace mli {

constexpr int kPromptMfmaRedPad = 4;   // floats between the parked rows: the four 16-lane rows of a store hit different banks
constexpr size_t prompt_mfma_work_bytes(int hd) {
    const size_t vt = kPlanWaves * gqa_mfma_vtile_bytes(hd), red = (size_t)kPlanWaves * 16 * (hd + kPromptMfmaRedPad) * sizeof(float);
    return vt > red ? vt : red;
}

// lgg = log2(g); window = 0: none, else 1 <= window < S (query t attends slots (t - window, t])
template <int HD, int NC>
__global__ __launch_bounds__(kFuThreads) void prompt_mfma_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ seg_row,
    const int* __restrict__ seg_first, const int* __restrict__ seg_count, const int* __restrict__ seg_offset,
    float* __restrict__ out, int n_blocks_per_seg, int n_q, int B, int S, int D, int Hkv, int lgg, int window) {
    static_assert(HD == 64 || HD == 128, "head_dim 64 or 128");
    constexpr int NM = HD / 32;             // score instructions per part and tile = 16-byte K loads = 16-byte V loads of a lane
    constexpr int NDT = HD / 16;            // 16-column tiles of the output
    constexpr int UPT = HD / 8;             // 16-byte units of a token's V head row
    constexpr int TPI = kWave / UPT;        // tokens one V load instruction covers
    constexpr int VSTRIDE = HD * 2 + 16;    // bytes of a token row of the V tile
    constexpr int RSTRIDE = HD + kPromptMfmaRedPad;   // floats of a parked column
    __shared__ __align__(16) unsigned char work[prompt_mfma_work_bytes(HD)];   // the waves' V tiles, then the parked columns
    __shared__ float2 wave_ml[kFuWaves * 16];

    const int g = 1 << lgg;
    const int tq = (NC * 16) >> lgg;
    int x = blockIdx.x;
    const int j = x % Hkv;
    x /= Hkv;
    const int seg = x / n_blocks_per_seg;
    const int j0 = (x % n_blocks_per_seg) * tq;   // the block's first query inside the segment
    const int cnt = seg_count[seg];
    if (j0 >= cnt) return;                        // surplus workgroup
    const int b = seg_row[seg], first_pos = seg_first[seg], off = seg_offset[seg];
    // a segment that does not lie inside the batch, the sequence and the q / out arrays is skipped whole
    if (b < 0 || b >= B || first_pos < 0 || (int64_t)first_pos + cnt > S || off < 0 || (int64_t)off + cnt > n_q) return;
    const int nq = min(tq, cnt - j0);
    const int t0 = first_pos + j0, t_hi = t0 + nq - 1;
    const int64_t q_row0 = (int64_t)off + j0;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n16 = lane & 15;   // scores: the lane's column of a tile; K: its token; output: its column of a 16-wide hd tile
    const int kg = lane >> 4;    // the 16-lane row: tokens 4 kg .. + 3 of the score tiles, run kg of a K head row
    const int W = S / kPage;

    // ---- the lane's columns: query position, first attended slot; q^T in three parts, in the B layout, once per block ----
    int tcol[NC], locol[NC];
    fu_u32x4 qp[NC][kMfmaParts][NM];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int col = c * 16 + n16, kq = col >> lgg, hh = col & (g - 1);
        const bool valid = kq < nq;
        tcol[c] = valid ? t0 + kq : -1;   // a surplus column attends nothing
        locol[c] = window > 0 ? max(0, tcol[c] + 1 - window) : 0;
        const float* qrow = q + (q_row0 + kq) * D + (j * g + hh) * HD + kg * (HD / 4);
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            uint32_t part[8][kMfmaParts];
#pragma unroll
            for (int e = 0; e < 8; ++e) mfma_split3(valid ? qrow[8 * i + e] : 0.f, part[e]);
#pragma unroll
            for (int p = 0; p < kMfmaParts; ++p) {
                qp[c][p][i].x = mfma_pack(part[0][p], part[1][p]);
                qp[c][p][i].y = mfma_pack(part[2][p], part[3][p]);
                qp[c][p][i].z = mfma_pack(part[4][p], part[5][p]);
                qp[c][p][i].w = mfma_pack(part[6][p], part[7][p]);
            }
        }
    }

    // the pages some query of the block attends
    const int lo0 = window > 0 ? max(0, t0 + 1 - window) : 0;   // first slot the block's first query attends
    const int p_lo = lo0 / kPage;
    const int nv = t_hi / kPage + 1 - p_lo;                      // >= 1, p_lo + nv <= W

    const float scale = sqrtf((float)HD);
    const float inv_scale = 1.f / scale;
    const int row_bytes = 3 * D * 2;                 // one token slot: x | K | V, bf16
    const int block_bytes = kPage * row_bytes;
    // K: token n16, run kg of K/V head j, one 16-byte unit per instruction.  V: TPI tokens per instruction, a head row coalesced
    const unsigned koff = (unsigned)(n16 * row_bytes + (D + j * HD + kg * (HD / 4)) * 2);
    const int vtok = lane / UPT, vunit = lane % UPT;
    const unsigned voff = (unsigned)(vtok * row_bytes + (2 * D + j * HD) * 2 + vunit * 16);
    unsigned char* vt = work + wave * gqa_mfma_vtile_bytes(HD);

    auto load_page = [&](int v, fu_u32x4 (&kr)[NM], fu_u32x4 (&vr)[NM]) {
        const char* pg = reinterpret_cast<const char*>(
            wave_uniform(reinterpret_cast<const float*>(page_table[(int64_t)b * W + p_lo + v])));
        // a null page gets an empty range: its loads return zeros; every offset below lies inside the page block
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(pg), 0, pg != nullptr ? block_bytes : 0, 0x00020000);
#pragma unroll
        for (int i = 0; i < NM; ++i) kr[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, koff, i * 16, 0);
#pragma unroll
        for (int i = 0; i < NM; ++i) vr[i] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, i * TPI * row_bytes, 0);
    };

    float run_m[NC], run_l[NC];   // of column n16 of tile c, the same bits in the column's four lanes
    mf_f32x4 acc[NC][NDT];        // columns 4 kg .. + 3 of tile c, output column n16 of hd tile dt
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        run_m[c] = -INFINITY;
        run_l[c] = 0.f;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) acc[c][dt] = mf_f32x4{0.f, 0.f, 0.f, 0.f};
    }

    fu_u32x4 kc[NM], vc[NM], kn[NM], vn[NM];   // the page being consumed and the wave's next one, in flight meanwhile
    if (wave < nv) load_page(wave, kc, vc);
    for (int v = wave; v < nv; v += kFuWaves) {
        const bool has_next = v + kFuWaves < nv;   // wave-uniform
        if (has_next) load_page(v + kFuWaves, kn, vn);
        const int first = (p_lo + v) * kPage;      // the page's first slot

        // ---- V tile -> LDS as loaded; a slot no query of the block attends as zeros ----
#pragma unroll
        for (int i = 0; i < NM; ++i) {
            const int t = i * TPI + vtok, s = first + t;
            const fu_u32x4 val = (s <= t_hi && s >= lo0) ? vc[i] : fu_u32x4{0u, 0u, 0u, 0u};
            *reinterpret_cast<fu_u32x4*>(vt + t * VSTRIDE + vunit * 16) = val;
        }
        __builtin_amdgcn_wave_barrier();   // other lanes of the wave read the tile back below: no LDS access moves across

        // ---- per column tile: scores^T (lo, mid, hi parts of q into one accumulator), mask, online softmax ----
        mf_s16x4 pa[NC][kMfmaParts];
        float al[NC][4];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            mf_f32x4 sc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p < kMfmaParts; ++p)
#pragma unroll
                for (int i = 0; i < NM; ++i)
                    sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(mf_bf16x8, kc[i]),
                                                                 __builtin_bit_cast(mf_bf16x8, qp[c][p][i]), sc, 0, 0, 0);
            // slot first + 4 kg + r is live for the column iff it lies in [locol, tcol]
            const int s0 = first + 4 * kg;
            float s[4];
            float pm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[r] = div_by(sc[r], scale, inv_scale);
                pm = (s0 + r <= tcol[c] && s0 + r >= locol[c]) ? fmaxf(pm, s[r]) : pm;
            }
            pm = fmaxf(pm, __shfl_xor(pm, 16, kWave));
            pm = fmaxf(pm, __shfl_xor(pm, 32, kWave));
            const float m_new = fmaxf(run_m[c], pm);
            // (no live slot yet: m_new is -inf too, and the state stays empty)
            const float alpha = run_m[c] == -INFINITY ? 0.f : expf(run_m[c] - m_new);
            float psum = 0.f;
            uint32_t pp[4][kMfmaParts];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float pr = (s0 + r <= tcol[c] && s0 + r >= locol[c]) ? expf(s[r] - m_new) : 0.f;
                psum += pr;
                mfma_split3(pr, pp[r]);
            }
            psum += __shfl_xor(psum, 16, kWave);
            psum += __shfl_xor(psum, 32, kWave);
            run_l[c] = run_l[c] * alpha + psum;
            run_m[c] = m_new;
            // the output tile holds columns 4 kg .. + 3: their alpha lives in lanes 4 kg .. + 3
#pragma unroll
            for (int r = 0; r < 4; ++r) al[c][r] = __shfl(alpha, 4 * kg + r, kWave);
#pragma unroll
            for (int p = 0; p < kMfmaParts; ++p)
                pa[c][p] = __builtin_bit_cast(mf_s16x4, mf_u32x2{mfma_pack(pp[0][p], pp[1][p]), mfma_pack(pp[2][p], pp[3][p])});
        }

        // ---- out += P . V: every V fragment read back transposed once, used by the NC column tiles ----
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            const unsigned short* colp = reinterpret_cast<const unsigned short*>(vt + (4 * kg) * VSTRIDE + (dt * 16 + n16) * 2);
            const uint32_t v0 = colp[0], v1 = colp[VSTRIDE / 2], v2 = colp[2 * (VSTRIDE / 2)], v3 = colp[3 * (VSTRIDE / 2)];
            const mf_s16x4 vb4 = __builtin_bit_cast(mf_s16x4, mf_u32x2{v0 | (v1 << 16), v2 | (v3 << 16)});
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                mf_f32x4 a = acc[c][dt];
#pragma unroll
                for (int r = 0; r < 4; ++r) a[r] *= al[c][r];
#pragma unroll
                for (int p = 0; p < kMfmaParts; ++p) a = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(pa[c][p], vb4, a, 0, 0, 0);
                acc[c][dt] = a;
            }
        }
        __builtin_amdgcn_wave_barrier();   // ... and the next page's tile is written only behind these reads
        if (has_next) {
#pragma unroll
            for (int i = 0; i < NM; ++i) {
                kc[i] = kn[i];
                vc[i] = vn[i];
            }
        }
    }

    // ---- the block's results, one column tile at a time: the waves (each owns whole pages) are merged in wave order ----
    float* red = reinterpret_cast<float*>(work);   // [waves][16 columns][RSTRIDE]
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        __syncthreads();   // the V tiles (first tile) or the previous tile's parked columns have been read
        if (kg == 0) wave_ml[wave * 16 + n16] = make_float2(run_m[c], run_l[c]);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[(wave * 16 + 4 * kg + r) * RSTRIDE + dt * 16 + n16] = acc[c][dt][r];
        __syncthreads();
        for (int i = threadIdx.x; i < 16 * (HD / 4); i += kFuThreads) {
            const int cr = i / (HD / 4), d = (i % (HD / 4)) * 4;
            const int col = c * 16 + cr, kq = col >> lgg, hh = col & (g - 1);
            if (kq >= nq) continue;   // a surplus column is never written
            float m = -INFINITY;
#pragma unroll
            for (int w = 0; w < kFuWaves; ++w) m = fmaxf(m, wave_ml[w * 16 + cr].x);
            float wsc[kFuWaves];
            float l = 0.f;
#pragma unroll
            for (int w = 0; w < kFuWaves; ++w) {
                const float2 st = wave_ml[w * 16 + cr];
                wsc[w] = st.x == -INFINITY ? 0.f : expf(st.x - m);
                l += st.y * wsc[w];
            }
            const float norm = 1.f / l;   // (a query attends itself at least: l > 0)
            float r4[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float t = 0.f;
#pragma unroll
                for (int w = 0; w < kFuWaves; ++w) t += red[(w * 16 + cr) * RSTRIDE + d + k] * wsc[w];
                r4[k] = t * norm;
            }
            *reinterpret_cast<float4*>(out + (q_row0 + kq) * D + (j * g + hh) * HD + d) = make_float4(r4[0], r4[1], r4[2], r4[3]);
        }
    }
}

// The launch for an accepted shape (prompt_mfma_shape_ok, prompt_mfma_grid_ok): window 0 = none.  n_seg >= 1, max_count >= 1.
inline int launch_prompt_mfma_scan(const float* q, const void* const* page_table, const int* seg_row, const int* seg_first,
                                   const int* seg_count, const int* seg_offset, float* out, int n_seg, int max_count, int n_q,
                                   int B, int S, int D, int H, int Hkv, int window, hipStream_t st) {
    const int hd = D / H, g = H / Hkv;
    const int lgg = g == 8 ? 3 : g == 4 ? 2 : g == 2 ? 1 : 0;
    const int tq = prompt_mfma_tq(hd, g), nc = tq * g / 16;
    const int nb = ceil_div_i(max_count, tq);
    if (!prompt_mfma_grid_ok(n_seg, Hkv, max_count, tq)) return MLI_ERR_BAD_ARG;   // (the entry points refuse it first)
    count_launch(kLfScanPromptMfma);
    const dim3 grid((unsigned)(n_seg * nb * Hkv)), block(kFuThreads);
    const auto go = [&](auto hdc, auto ncc) {
        hipLaunchKernelGGL((prompt_mfma_scan_kernel<decltype(hdc)::value, decltype(ncc)::value>), grid, block, 0, st, q, page_table,
                           seg_row, seg_first, seg_count, seg_offset, out, nb, n_q, B, S, D, Hkv, lgg, window);
    };
    using std::integral_constant;
    if (hd == 128) {   // (prompt_mfma_max_tiles: four tiles at head_dim 128 do not compile without scratch)
        if (nc == 2) go(integral_constant<int, 128>{}, integral_constant<int, 2>{});
        else go(integral_constant<int, 128>{}, integral_constant<int, 1>{});
    } else {
        if (nc == 4) go(integral_constant<int, 64>{}, integral_constant<int, 4>{});
        else if (nc == 2) go(integral_constant<int, 64>{}, integral_constant<int, 2>{});
        else go(integral_constant<int, 64>{}, integral_constant<int, 1>{});
    }
    return launch_status();
}

}  // namespace mli
