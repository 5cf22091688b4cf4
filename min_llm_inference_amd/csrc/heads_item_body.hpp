// Multi-head form of the single-pass scan's workgroup body (scan_item_body.hpp: fused_scan_item, whole pages per wave,
// lean mode, in-kernel merge).  Head h owns columns [h * hd, (h + 1) * hd) of q and of the K and V segments; one softmax
// per head over q_h . K_h / sqrtf(hd).  The bytes loaded and the way they are loaded are fused_scan_item's; what differs is
// what happens between a page's K batches and its V batches, and that every statistic exists once per head.
//
// Lanes and heads.  A lane's 16-byte unit u (EPL elements) lies inside head u * EPL / hd because hd is a multiple of EPL,
// so head h is a GROUP of G = hd / EPL consecutive lanes (a power of two, 4 .. 64) of one load instruction; with two lane
// loads per row (NJ = 2) the two units of a lane belong to different heads.  All softmax state is therefore kept per lane
// and per j: the running (max, sum) and the page's 16 probabilities of the lane's own head.  The 16 partial scores are
// summed by an xor butterfly over the log2 G distances below G -- the exchanges between groups are the ones to skip, the
// groups hold different heads -- which leaves every lane of a group with bit-identical scores (a + b == b + a), so the
// lanes of a head agree on every later value without a broadcast, and nothing is wave-uniform any more.
#pragma once

#include "scan_item_body.hpp"
#include "scan_plan.hpp"

namespace mli {

// x / d for a divisor whose reciprocal r = 1 / d is at hand: one Newton correction of the product (the residual is
// exact in the fma), within half an ulp of the quotient like the division it replaces -- 16 scores per lane and page.
__device__ __forceinline__ float div_by(float x, float d, float r) {
    const float qt = x * r;
    return fmaf(fmaf(-qt, d, x), r, qt);
}

// EXTENSION (attention_softcap.hpp): logit soft-capping, cap * tanh(x / cap) of a scaled score x; cap > 0 finite, r = 1 / cap.
// The one evaluation of the cap on the device: the multi-head decode scan below and the prompt scan (attention_prompt.hpp) call
// it between div_by and the page maximum, and nothing else does.  u = x / cap by div_by (half an ulp).  Below |u| = 0.5 an odd
// polynomial u + u^3 P(u^2) (degree 4 in u^2, fitted at Chebyshev nodes; 1.1 * 2^-24 relative in fp32, and exactly u where u^3
// vanishes beside u: the value is accurate RELATIVE to the score however small the score is beside the cap); from 0.5 on
// 1 - 2 / (e^{2|u|} + 1) with the sign of u, whose absolute error of about 2^-24 is then relative too (tanh >= 0.46; 3.5 * 2^-24
// measured).  Both are computed and one select picks: no branch, no table, two transcendental instructions.  e^{2|u|} = inf
// gives 1 exactly; a NaN score stays NaN (the mask drops dead slots AFTER the cap, by select: tanh(-inf) = -1 never gets
// the chance to make a dead slot a finite -cap).  Contraction is off inside: the closing product must be ROUNDED before the
// softmax subtracts the maximum from it -- fused into that subtraction, a row's only score minus itself is no longer 0 and a row
// of one token no longer returns V's row bit for bit.  (The fmaf calls are fused by their own text.)
__device__ __forceinline__ float softcap_score(float x, float cap, float r) {
#pragma clang fp contract(off)
    const float u = div_by(x, cap, r);
    const float a = fabsf(u);
    const float z = u * u;
    float p = fmaf(-0.00694699864834547f, z, 0.021472718566656113f);
    p = fmaf(p, z, -0.05393378809094429f);
    p = fmaf(p, z, 0.1333322674036026f);
    p = fmaf(p, z, -0.3333333134651184f);
    const float lo = fmaf(u * z, p, u);
    const float e = __expf(2.f * a);
    const float hi = copysignf(fmaf(-2.f, __builtin_amdgcn_rcpf(e + 1.f), 1.f), u);
    return cap * (a < 0.5f ? lo : hi);
}

// The partner's value for one step of the all-reduce inside a lane group.  Distances 1 and 2 are DPP quad permutes; 4 and
// 8 are the DPP mirrors of 8 and 16 lanes (lane i <-> 7 - i, i <-> 15 - i): after the earlier steps every lane of the
// smaller group holds the same value, so the mirror pairs the same two groups the xor would.  No LDS crossbar trip and no
// address register for these; 16 and 32 take the wave shuffle.
template <int DIST>
__device__ __forceinline__ float heads_partner(float x) {
    if constexpr (DIST <= 8) {
        constexpr int ctrl = DIST == 1 ? 0xB1 : DIST == 2 ? 0x4E : DIST == 4 ? 0x141 : 0x140;
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), ctrl, 0xf, 0xf, true));
    } else {
        return __shfl_xor(x, DIST, kWave);
    }
}

// v[j][t] += the same element of the partner lanes at distance DIST (steps in rising order of DIST), for both lane loads
template <int NJ, int DIST>
__device__ __forceinline__ void heads_xor_step(float (&v)[NJ][16]) {
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int t = 0; t < 16; ++t) v[j][t] += heads_partner<DIST>(v[j][t]);
}

// lg = log2 G (2 .. 6), H = heads.  arrivals: the rows' arrival counters (used when the row has several items).
// ml: [B][nchunk_max][H] (max, sum) per item and head; partial: [B][nchunk_max][D] un-normalised partial rows.
// TBR = rows per load batch, PD = batches in flight (of four register buffers).
// smem_raw: ct / 16 page pointers | max(4 waves x (NJ * 64 * EPL floats + NJ * 64 float2), nchunk_max * H float2)
// WIN = true (EXTENSION, attention_heads.hpp): the row attends its newest `window` tokens -- fused_scan_item's window
// switch: the row is taken from its first live page p0 on, and that page's slots below the window are masked.
// SINK = true (EXTENSION, attention_heads.hpp; with WIN): fused_scan_item's sink switch -- the first n_sink tokens are attended
// too, on the virtual row of sink pages + window pages; the mask is per slot of the lane's 16.
// GQA = true (EXTENSION, attention_heads.hpp): grouped-query attention, gq = n_heads / n_kv_heads query heads per K/V head.  Only
// the unit a lane LOADS changes (gqa_kv_unit, scan_plan.hpp): the lanes of query head h read the K and V columns of K/V head
// h / gq.  q, the per-lane state, the all-reduce inside a group, the merges and H are those of n_heads heads.
// ALIBI = true (EXTENSION, attention_alibi.hpp): a linear position bias per query head, slopes[h] * (s - (L_row - 1)) added to
// the scaled score of the row's absolute slot s -- 0 at the newest token.  A lane keeps the slope of its own head per lane
// load; the bias is one fmaf between div_by and the page maximum, on the page's first absolute slot, which the body has
// already.  The bias is absolute in the row, so the (m, l) of a row's items live in one frame and the merges do not change.
// SOFTCAP = true (EXTENSION, attention_softcap.hpp; never with ALIBI): logit soft-capping, the scaled score x becomes
// cap * tanh(x / cap) (softcap_score) at the same place, between div_by and the page maximum; cap is a kernel argument.  A
// pure function of the score: masks, (m, l) frames and merges do not change, and a masked slot stays masked.
// SINKLOGIT = true (EXTENSION, attention_sink_logits.hpp; never with ALIBI or SOFTCAP): a learned attention-sink logit per QUERY
// head, sink_logits[h] (n_heads floats in device memory, each finite or -inf).  It takes part in head h's softmax as one more
// logit without a value row: m = max(m, z) and l += exp(z - m), exactly once per (row, head).  So it enters only where a row's
// FINAL (m, l) of a head is formed -- the wave merge of a row with one workgroup (direct), or the last arriver's merge over the
// items -- and never what an item publishes.  The maximum takes the sink in BEFORE any exp of a difference (a logit far above
// every score gives zeros, not inf / NaN); z = -inf leaves m and l as they were, bit for bit (fmaxf(m, -inf) = m, l + 0 = l).
// The page loop, the prefetch, the plan, the workspace, the LDS size and the arrival counters do not change.
template <class E, int NJ, bool NT, int TBR, int PD, bool WIN = false, bool SINK = false, bool GQA = false, bool ALIBI = false,
          bool SOFTCAP = false, bool SINKLOGIT = false>
__device__ __forceinline__ void heads_scan_item(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ out, float2* ml, float* partial, int S, int D, int lg, int H, int ct, int nchunk_max, int direct,
    unsigned* arrivals, int b, int c, bool first_grid_row, unsigned char* smem_raw, int window = 0, int n_sink = 0,
    int gq = 1, const float* __restrict__ slopes = nullptr, float cap = 0.f, const float* __restrict__ sink_logits = nullptr) {
    static_assert(!SINK || WIN, "sinks exist beside a window only");
    static_assert(!(ALIBI && SOFTCAP), "the order of bias and cap would be an invention");
    static_assert(!(SINKLOGIT && (ALIBI || SOFTCAP)), "no model defines a sink logit beside a position bias or a cap");
    constexpr int EPL = E::EPL;
    constexpr int kRowF = NJ * kWave * EPL;   // floats one wave parks
    constexpr int kRowU = NJ * kWave;         // lane units of a row
    const void** ptr_sh = reinterpret_cast<const void**>(smem_raw);                      // ct/16 page pointers
    float* red = reinterpret_cast<float*>(smem_raw + (size_t)(ct / kPage) * 8);           // [waves][kRowF]
    float2* wave_ml = reinterpret_cast<float2*>(red + kFuWaves * kRowF);                 // [waves][kRowU]
    __shared__ int last_sh;

    // prologue chain as in fused_scan_item: the full-chunk grid rows ask for their page pointers before the length is known
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x >> 6;
    const int W = S / kPage;
    const bool early = !WIN && c < nchunk_max;   // (a windowed row's first page depends on its length)
    const void* early_ptr = nullptr;
    if (early && (int)threadIdx.x < ct / kPage && c * (ct / kPage) + (int)threadIdx.x < W)
        early_ptr = page_table[(int64_t)b * W + c * (ct / kPage) + threadIdx.x];
    const int Du = D / EPL;  // lane units per row
    float qr[NJ][EPL];
    unsigned voff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int u = lane + j * kWave;
        const bool live = u < Du;   // dead lanes come in whole groups (Du = H * G): they score zeros nobody reads
        // lanes beyond the row get an offset outside the page block: the buffer range check returns zeros for them
        // (the old statement stays verbatim in the else branch, as for SINK below)
        if constexpr (GQA) voff[j] = live ? (unsigned)gqa_kv_unit(u, lg, gq) * 16u : 0x40000000u;
        else voff[j] = live ? (unsigned)u * 16u : 0x40000000u;
#pragma unroll
        for (int e = 0; e < EPL; ++e) qr[j][e] = live ? q[(int64_t)b * D + u * EPL + e] : 0.f;
    }
    float slope[NJ];   // ALIBI: the slope of the lane's head per lane load (dead lanes: no head, nothing read)
    if constexpr (ALIBI) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) slope[j] = lane + j * kWave < Du ? slopes[(lane + j * kWave) >> lg] : 0.f;
    }
    const int L_row = min(lengths[b], S);
    const int lo = WIN ? max(0, L_row - window) : 0;   // first slot the row attends
    const int p0 = lo / kPage;                         // ... and the page it lies in
    const int ps = SINK ? (n_sink + kPage - 1) / kPage : 0;   // sink pages
    const int skip = SINK ? max(0, p0 - ps) : p0;             // pages dropped in front of the window's first page
    const int L = L_row - skip * kPage;                // the row from that page on (SINK: the virtual row)
    if (L <= 0) {
        // no workgroup arrives for an empty row: its zero result is written here, once
        if (first_grid_row)
            for (int i = threadIdx.x; i < D; i += kFuThreads) out[(int64_t)b * D + i] = 0.f;
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
    const int npages = (ntok + kPage - 1) / kPage;
    if (early) {
        if ((int)threadIdx.x < npages) ptr_sh[threadIdx.x] = early_ptr;   // npages <= ct / 16 <= 64 < threads
    } else {
        for (int i = threadIdx.x; i < npages; i += kFuThreads) {
            // (the old statement stays verbatim in the else branch: folded into one expression with a SINK operand, the
            // 64-bit address sum of the existing kernels re-associates and their device code changes)
            if constexpr (SINK) ptr_sh[i] = page_table[(int64_t)b * W + sink_page(s0 / kPage + i, ps, skip)];
            else ptr_sh[i] = page_table[(int64_t)b * W + p0 + s0 / kPage + i];
        }
    }
    __syncthreads();

    const float scale = sqrtf((float)(EPL << lg));   // sqrtf(head_dim)
    const float inv_scale = 1.f / scale;
    const float inv_cap = SOFTCAP ? 1.f / cap : 0.f;
    const int64_t row_bytes = (int64_t)3 * D * E::kBytes;
    const int64_t seg_bytes = (int64_t)D * E::kBytes;

    float run_m[NJ], run_l[NJ];
    float acc[NJ][EPL];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        run_m[j] = -INFINITY;
        run_l[j] = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[j][e] = 0.f;
    }
    // the rolling prefetch of fused_scan_item: batch `pos` of every page lives in register buffer pos % NBUF, and before it
    // is consumed batch pos + PD -- of this page or of the wave's next page -- is issued.  NBUF divides the batches of a
    // page, so the buffer index stays in step across the page boundary (batch NPOS + k of this page IS batch k of the
    // next one), and PD < NBUF, so a batch is never issued into the buffer being consumed or one still waiting.  With
    // PD = 2 only three of the four buffers are live at any point: that is what the register allocator sees.
    constexpr int NB = 16 / TBR;
    constexpr int NPOS = 2 * NB;
    constexpr int NBUF = 4;
    static_assert(NPOS % NBUF == 0, "the buffer index must stay in step across the page boundary");
    static_assert(PD >= 1 && PD < NBUF, "a batch in flight may not share a buffer with one not yet consumed");
    fu_u32x4 buf[NBUF][TBR][NJ];
    const int block_bytes = kPage * 3 * D * E::kBytes;
    auto page_ptr = [&](int pi) {
        return reinterpret_cast<const char*>(wave_uniform(reinterpret_cast<const float*>(ptr_sh[pi])));
    };
    auto issue = [&](auto POS, const char* pg) {
        constexpr int pos = decltype(POS)::value;
        constexpr int bi = pos % NBUF;
        const char* upg = reinterpret_cast<const char*>(wave_uniform(reinterpret_cast<const float*>(pg)));
        // a null page gets an empty range: its loads return zeros
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(upg), 0, upg != nullptr ? block_bytes : 0, 0x00020000);
        const int base = (pos < NB ? (int)seg_bytes : 2 * (int)seg_bytes) + (pos % NB) * TBR * (int)row_bytes;
#pragma unroll
        for (int t = 0; t < TBR; ++t)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                buf[bi][t][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[j], base + t * (int)row_bytes, NT ? 2 : 0);
    };

    const char* page = wave < npages ? page_ptr(wave) : nullptr;
    if (wave < npages) {
        static_for<PD>([&](auto POS) { issue(POS, page); });
    }
    for (int pi = wave; pi < npages; pi += kFuWaves) {
        const bool has_next = pi + kFuWaves < npages;
        const char* next = has_next ? page_ptr(pi + kFuWaves) : nullptr;
        const int nt = min(kPage, ntok - pi * kPage);  // live tokens in this page (>= 1)
        int nlo = (WIN && pi == 0 && s0 == 0) ? lo - p0 * kPage : 0;   // slots below the window (row's first live page)
        int nk = 0;                                                         // slots among the sinks
        // (SINK overwrites the nlo above, which is dead there: the line stays as it was so that the existing kernels' device
        // code does not change)
        if constexpr (SINK) {
            const int first = sink_page(s0 / kPage + pi, ps, skip) * kPage;   // the page's first slot in the row
            nlo = lo - first;
            nk = n_sink - first;
        }
        // ALIBI: the page's first slot relative to the row's newest token; (float)int + (float)t is exact below 2^24
        float rel0 = 0.f;
        if constexpr (ALIBI) {
            int first_abs;
            if constexpr (SINK) first_abs = sink_page(s0 / kPage + pi, ps, skip) * kPage;
            else first_abs = kPage * (skip + s0 / kPage + pi);
            rel0 = (float)(first_abs - (L_row - 1));
        }
        float sp[NJ][16];   // partial scores, then scores, then the page's probabilities (of the lane's head for j)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int t = 0; t < 16; ++t) sp[j][t] = 0.f;

        static_for<NPOS>([&](auto POS) {
            constexpr int pos = decltype(POS)::value;
            constexpr int bi = pos % NBUF;
            constexpr int tgt = pos + PD;
            if constexpr (tgt < NPOS) {
                issue(std::integral_constant<int, tgt>{}, page);
            } else {
                if (has_next) issue(std::integral_constant<int, tgt - NPOS>{}, next);  // wave-uniform
            }
            if constexpr (pos < NB) {
                // ---- K batch: this lane's part of the scores of slots pos*TBR .. pos*TBR+TBR-1 ----
#pragma unroll
                for (int t = 0; t < TBR; ++t)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) ElemMath<E>::dot(buf[bi][t][j], qr[j], sp[j][pos * TBR + t]);
                if constexpr (pos == NB - 1) {
                    // complete the dot products inside each head's lane group (lg is wave-uniform)
                    heads_xor_step<NJ, 1>(sp);
                    heads_xor_step<NJ, 2>(sp);
                    if (lg > 2) heads_xor_step<NJ, 4>(sp);
                    if (lg > 3) heads_xor_step<NJ, 8>(sp);
                    if (lg > 4) heads_xor_step<NJ, 16>(sp);
                    if (lg > 5) heads_xor_step<NJ, 32>(sp);
                    // online softmax update per head (slots >= nt hold allocated but meaningless data: masked here)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        float pm = -INFINITY;
#pragma unroll
                        for (int t = 0; t < 16; ++t) {
                            sp[j][t] = div_by(sp[j][t], scale, inv_scale);
                            if constexpr (ALIBI) sp[j][t] = fmaf(slope[j], rel0 + (float)t, sp[j][t]);
                            if constexpr (SOFTCAP) sp[j][t] = softcap_score(sp[j][t], cap, inv_cap);
                            pm = slot_live<WIN, SINK>(t, nt, nlo, nk) ? fmaxf(pm, sp[j][t]) : pm;
                        }
                        const float m_new = fmaxf(run_m[j], pm);
                        const float alpha = run_m[j] == -INFINITY ? 0.f : expf(run_m[j] - m_new);
                        float psum = 0.f;
#pragma unroll
                        for (int t = 0; t < 16; ++t) {
                            sp[j][t] = slot_live<WIN, SINK>(t, nt, nlo, nk) ? expf(sp[j][t] - m_new) : 0.f;
                            psum += sp[j][t];
                        }
                        run_l[j] = run_l[j] * alpha + psum;
                        run_m[j] = m_new;
#pragma unroll
                        for (int e = 0; e < EPL; ++e) acc[j][e] *= alpha;
                    }
                }
            } else {
                // ---- V batch: acc += p . V over the live slots, each lane with its own head's probability ----
                constexpr int first = (pos - NB) * TBR;
#pragma unroll
                for (int t = 0; t < TBR; ++t) {
                    // wave-uniform: never multiply unwritten page memory (or a slot below the window), even by zero
                    if (slot_live<WIN, SINK>(first + t, nt, nlo, nk)) {
#pragma unroll
                        for (int j = 0; j < NJ; ++j) ElemMath<E>::axpy(buf[bi][t][j], sp[j][first + t], acc[j]);
                    }
                }
            }
        });
        page = next;
    }

    // ---- the item's result per head: the waves (each owns whole pages) are merged in wave order through LDS ----
    const bool publish = !direct;
    float* o = direct ? out + (int64_t)b * D : partial + ((int64_t)b * nchunk_max + c) * D;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        wave_ml[wave * kRowU + j * kWave + lane] = make_float2(run_m[j], run_l[j]);
#pragma unroll
        for (int e = 0; e < EPL; ++e) red[wave * kRowF + (j * kWave + lane) * EPL + e] = acc[j][e];
    }
    __syncthreads();
    const __amdgpu_buffer_rsrc_t orow = __builtin_amdgcn_make_buffer_rsrc(o, 0, D * (int)sizeof(float), 0x00020000);
    const int hd_shift = lg + (EPL == 8 ? 3 : 2);   // log2 head_dim
    // element i of the row lives at red[...][i]; the four elements of a thread share a lane unit, hence a head
    for (int i = 4 * threadIdx.x; i < D; i += 4 * kFuThreads) {
        const int u = i / EPL;
        float m = -INFINITY;
#pragma unroll
        for (int w = 0; w < kFuWaves; ++w) m = fmaxf(m, wave_ml[w * kRowU + u].x);
        // SINKLOGIT, a row of one workgroup: this IS the row's final (m, l).  The four elements of a thread share a head, so
        // they share z; the sink joins the maximum before the waves' weights are formed.  (An item that publishes keeps -inf.)
        float zsink = -INFINITY;
        if constexpr (SINKLOGIT) {
            if (direct) {
                zsink = sink_logits[i >> hd_shift];
                m = fmaxf(m, zsink);
            }
        }
        float wsc[kFuWaves];
        float l = 0.f;
#pragma unroll
        for (int w = 0; w < kFuWaves; ++w) {
            const float2 s = wave_ml[w * kRowU + u];
            wsc[w] = s.x == -INFINITY ? 0.f : expf(s.x - m);
            l += s.y * wsc[w];
        }
        if constexpr (SINKLOGIT) {
            if (direct) l += expf(zsink - m);   // the sink's share of the denominator; it has no value row
        }
        const float norm = direct ? 1.f / l : 1.f;
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < kFuWaves; ++w) t += red[w * kRowF + i + k] * wsc[w];
            r[k] = t * norm;
        }
        if (publish) {
            // write-through (sc1) stores: another workgroup may read the row back inside this launch
            fu_u32x4 raw;
            raw.x = __float_as_uint(r[0]); raw.y = __float_as_uint(r[1]); raw.z = __float_as_uint(r[2]); raw.w = __float_as_uint(r[3]);
            __builtin_amdgcn_raw_buffer_store_b128(raw, orow, i * (int)sizeof(float), 0, 16);
            if ((i & ((1 << hd_shift) - 1)) == 0) {   // the head's first element: its (m, l) goes with it
                typedef unsigned long long __attribute__((address_space(1)))* gu64_ptr;
                const unsigned long long packed = ((unsigned long long)__float_as_uint(l) << 32) | __float_as_uint(m);
                __hip_atomic_store((gu64_ptr)(ml + ((int64_t)b * nchunk_max + c) * H + (i >> hd_shift)), packed,
                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // sc1 store
            }
        } else {
            *reinterpret_cast<float4*>(o + i) = make_float4(r[0], r[1], r[2], r[3]);
        }
    }
    if (!publish) return;

    // ---- count the arrival; the workgroup that completes the row merges its items per head, in item order ----
    const int nc = (L + ct - 1) / ct;
    if (!row_arrive(arrivals + b, nc, &last_sh)) return;
    typedef unsigned long long __attribute__((address_space(1)))* gu64_ptr;
    float2* ml_sh = reinterpret_cast<float2*>(red);   // [nc][H]; the barriers of row_arrive lie behind the last read of red
    const float2* ml_row = ml + (int64_t)b * nchunk_max * H;
    for (int i = threadIdx.x; i < nc * H; i += kFuThreads) {
        const unsigned long long packed = __hip_atomic_load((gu64_ptr)(ml_row + i), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ml_sh[i] = make_float2(__uint_as_float((unsigned)packed), __uint_as_float((unsigned)(packed >> 32)));
    }
    __syncthreads();
    const float* partial_row = partial + (int64_t)b * nchunk_max * D;
    float* out_row = out + (int64_t)b * D;
    for (int d = 4 * threadIdx.x; d < D; d += 4 * kFuThreads) {
        const int h = d >> hd_shift;
        float mm = -INFINITY;
        for (int i = 0; i < nc; ++i) mm = fmaxf(mm, ml_sh[i * H + h].x);
        // SINKLOGIT: the row's final (m, l) over its items -- the sink joins the maximum first, then the sum, once
        float zsink = -INFINITY;
        if constexpr (SINKLOGIT) {
            zsink = sink_logits[h];
            mm = fmaxf(mm, zsink);
        }
        float ll = 0.f;
        for (int i = 0; i < nc; ++i) ll = fmaf(ml_sh[i * H + h].y, expf(ml_sh[i * H + h].x - mm), ll);
        if constexpr (SINKLOGIT) ll += expf(zsink - mm);
        const float inv_l = 1.f / ll;
        float r[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = 0; i0 < nc; i0 += 8) {   // up to 8 partial rows in flight
            fu_u32x4 v[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (i0 + k < nc) {
                    const float* row_i = partial_row + (int64_t)(i0 + k) * D;
                    const __amdgpu_buffer_rsrc_t prow =
                        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(row_i), 0, D * (int)sizeof(float), 0x00020000);
                    v[k] = __builtin_amdgcn_raw_buffer_load_b128(prow, d * (int)sizeof(float), 0, 16);   // sc1: never L1
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (i0 + k < nc) {
                    const float w = expf(ml_sh[(i0 + k) * H + h].x - mm);
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

}  // namespace mli
