// The kernel of the causal multi-query prompt scan (attention_prompt.hpp has the account), included three times by that file:
//   MLI_PROMPT_SOFTCAP 0   prompt_scan_kernel<E, NJ, TQ, HEADS>, the text the kernel has always had;
//   MLI_PROMPT_SOFTCAP 1   prompt_softcap_scan_kernel<E, NJ, TQ> (EXTENSION, attention_softcap.hpp; several heads only): logit
//                          soft-capping, every scaled score x becomes cap * tanh(x / cap) (softcap_score, heads_item_body.hpp)
//                          between div_by and the page maximum, as in the decode scan -- query t of a segment gets what the
//                          capped decode scan gives a row of length t + 1.  One more argument: float cap.
//   MLI_PROMPT_SINK_LOGITS 1   (with MLI_PROMPT_SOFTCAP 0) prompt_sink_logits_scan_kernel<E, NJ, TQ> (EXTENSION,
//                          attention_sink_logits.hpp; several heads only): a learned sink logit per query head joins the maximum
//                          and the denominator where a query's final (m, l) is formed -- the wave merge, in front of the norm.
//                          One more argument: const float* sink_logits (n_heads floats in device memory).
// Three kernels of one text, so that the kernel with the switch has a name of its own and the kernels without it keep their
// symbols and their device code (a body shared through a device function moves their early exits and with them the registers).
// No include guard.

// lg: log2 lanes per head (HEADS), gq = n_heads / n_kv_heads (HEADS; 1 = no grouping); window 0 = none (then n_sink 0)
#if MLI_PROMPT_SINK_LOGITS
template <class E, int NJ, int TQ>
__global__ __launch_bounds__(kFuThreads) void prompt_sink_logits_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ seg_row,
    const int* __restrict__ seg_first, const int* __restrict__ seg_count, const int* __restrict__ seg_offset,
    float* __restrict__ out, int n_blocks_per_seg, int n_q, int B, int S, int D, int lg, int gq, int window, int n_sink,
    const float* __restrict__ sink_logits) {
    constexpr bool HEADS = true;
#elif MLI_PROMPT_SOFTCAP
template <class E, int NJ, int TQ>
__global__ __launch_bounds__(kFuThreads) void prompt_softcap_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ seg_row,
    const int* __restrict__ seg_first, const int* __restrict__ seg_count, const int* __restrict__ seg_offset,
    float* __restrict__ out, int n_blocks_per_seg, int n_q, int B, int S, int D, int lg, int gq, int window, int n_sink,
    float cap) {
    constexpr bool HEADS = true;
#else
template <class E, int NJ, int TQ, bool HEADS>
__global__ __launch_bounds__(kFuThreads) void prompt_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ seg_row,
    const int* __restrict__ seg_first, const int* __restrict__ seg_count, const int* __restrict__ seg_offset,
    float* __restrict__ out, int n_blocks_per_seg, int n_q, int B, int S, int D, int lg, int gq, int window, int n_sink) {
#endif
    constexpr int EPL = E::EPL;
    constexpr int kRowF = NJ * kWave * EPL;   // floats one wave parks per query
    constexpr int kRowU = NJ * kWave;         // lane units of a row
    __shared__ float red[kFuWaves * kRowF];
    __shared__ float2 wave_ml[kFuWaves * kRowU];

    const int seg = blockIdx.x / n_blocks_per_seg;
    const int j0 = (blockIdx.x % n_blocks_per_seg) * TQ;   // the block's first query inside the segment
    const int cnt = seg_count[seg];
    if (j0 >= cnt) return;                                  // surplus workgroup
    const int b = seg_row[seg], first_pos = seg_first[seg], off = seg_offset[seg];
    // a segment that does not lie inside the batch, the sequence and the q / out arrays is skipped whole
    if (b < 0 || b >= B || first_pos < 0 || (int64_t)first_pos + cnt > S || off < 0 || (int64_t)off + cnt > n_q) return;
    const int nq = min(TQ, cnt - j0);
    const int t0 = first_pos + j0, t_hi = t0 + nq - 1;
    const int64_t q_row0 = (int64_t)off + j0;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int W = S / kPage;
    const int Du = D / EPL;   // lane units per row
    float qr[TQ][NJ][EPL];
    unsigned voff[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int u = lane + j * kWave;
        const bool live = u < Du;   // (several heads: dead lanes come in whole groups and score zeros nobody reads)
        // lanes beyond the row get an offset outside the page block: the buffer range check returns zeros for them
        voff[j] = live ? (unsigned)(HEADS ? gqa_kv_unit(u, lg, gq) : u) * 16u : 0x40000000u;
#pragma unroll
        for (int k = 0; k < TQ; ++k)
#pragma unroll
            for (int e = 0; e < EPL; ++e) qr[k][j][e] = (live && k < nq) ? q[(q_row0 + k) * D + u * EPL + e] : 0.f;
    }
    // The pages some query of the block attends: the sink pages, then those from the first query's window on -- the virtual
    // row of scan_item_body.hpp (SINK), cut for the block: ps sink pages, `skip` dropped, nv pages in all.
    const int lo0 = window > 0 ? max(0, t0 + 1 - window) : 0;   // first slot the block's first query attends
    const int p_lo = lo0 / kPage;
    const int ps = min((n_sink + kPage - 1) / kPage, p_lo);
    const int skip = p_lo - ps;
    const int nv = t_hi / kPage + 1 - skip;

    const float scale = HEADS ? sqrtf((float)(EPL << lg)) : sqrtf((float)D);
    const float inv_scale = 1.f / scale;
    #if MLI_PROMPT_SOFTCAP
    const float inv_cap = 1.f / cap;
#endif
    const int row_bytes = 3 * D * E::kBytes;   // consecutive token slots of a page
    const int seg_bytes = D * E::kBytes;       // segment stride inside a slot: x | K | V

    constexpr int NS = HEADS ? NJ : 1;   // softmax states per query a lane keeps
    float run_m[TQ][NS], run_l[TQ][NS];
    float acc[TQ][NJ][EPL];
#pragma unroll
    for (int k = 0; k < TQ; ++k) {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            run_m[k][s] = -INFINITY;
            run_l[k][s] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int e = 0; e < EPL; ++e) acc[k][j][e] = 0.f;
    }

    // the rolling prefetch of the decode scans: batch `pos` of every page lives in register buffer pos % NBUF, and before it
    // is consumed batch pos + PD -- of this page or of the wave's next page -- is issued
    constexpr int TBR = NJ == 1 ? 4 : 2;
    constexpr int NB = 16 / TBR;
    constexpr int NPOS = 2 * NB;
    constexpr int NBUF = 4;
    constexpr int PD = (HEADS && NJ == 2 && EPL == 8) ? 2 : 3;   // (heads_decode_scan_kernel: the same variant, the same reason)
    static_assert(NPOS % NBUF == 0, "the buffer index must stay in step across the page boundary");
    fu_u32x4 buf[NBUF][TBR][NJ];
    const int block_bytes = kPage * 3 * D * E::kBytes;
    auto page_ptr = [&](int v) {
        return reinterpret_cast<const char*>(
            wave_uniform(reinterpret_cast<const float*>(page_table[(int64_t)b * W + sink_page(v, ps, skip)])));
    };
    auto issue = [&](auto POS, const char* pg) {
        constexpr int pos = decltype(POS)::value;
        constexpr int bi = pos % NBUF;
        const char* upg = reinterpret_cast<const char*>(wave_uniform(reinterpret_cast<const float*>(pg)));
        // a null page gets an empty range: its loads return zeros
        const __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(upg), 0, upg != nullptr ? block_bytes : 0, 0x00020000);
        const int base = (pos < NB ? seg_bytes : 2 * seg_bytes) + (pos % NB) * TBR * row_bytes;
#pragma unroll
        for (int t = 0; t < TBR; ++t)
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                buf[bi][t][j] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff[j], base + t * row_bytes, 0);
    };

    const char* page = wave < nv ? page_ptr(wave) : nullptr;
    if (wave < nv) {
        static_for<PD>([&](auto POS) { issue(POS, page); });
    }
    for (int v = wave; v < nv; v += kFuWaves) {
        const bool has_next = v + kFuWaves < nv;
        const char* next = has_next ? page_ptr(v + kFuWaves) : nullptr;
        // the page's slots, per query k: nt[k] inside the query's causal range (<= 0 for a surplus query of the last block),
        // nlo[k] below its window, nk among the sinks -- slot_live's operands
        const int first = sink_page(v, ps, skip) * kPage;
        const int nk = n_sink - first;
        int nt[TQ], nlo[TQ];
#pragma unroll
        for (int k = 0; k < TQ; ++k) {
            const int t = k < nq ? t0 + k : -1;
            nt[k] = t + 1 - first;
            nlo[k] = (window > 0 ? max(0, t + 1 - window) : 0) - first;
        }
        // partial scores, then (several heads) scores, then the page's probabilities of the lane's head
        float sp[TQ][NS][16];
        float p_lane[TQ];   // one head: the probability of slot (lane >> 2) & 15
#pragma unroll
        for (int k = 0; k < TQ; ++k) {
            p_lane[k] = 0.f;
#pragma unroll
            for (int s = 0; s < NS; ++s)
#pragma unroll
                for (int t = 0; t < 16; ++t) sp[k][s][t] = 0.f;
        }

        static_for<NPOS>([&](auto POS) {
            constexpr int pos = decltype(POS)::value;
            constexpr int bi = pos % NBUF;
            constexpr int tgt = pos + PD;
            if constexpr (tgt < NPOS) {
                issue(std::integral_constant<int, tgt>{}, page);
            } else {
                if (has_next) issue(std::integral_constant<int, tgt - NPOS>{}, next);  // wave-uniform
            }
            // keep the batch's loads HERE: with TQ queries' state live, loads hoisted to the top of the page (nothing but
            // register pressure orders them) cost more registers than the whole rolling buffer
            asm volatile("" ::: "memory");
            if constexpr (pos < NB) {
                // ---- K batch: every unit is unpacked once and dotted with the TQ query vectors ----
#pragma unroll
                for (int t = 0; t < TBR; ++t)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) {
                        float f[EPL];
                        E::unpack(buf[bi][t][j], f);
#pragma unroll
                        for (int k = 0; k < TQ; ++k)
#pragma unroll
                            for (int e = 0; e < EPL; ++e)
                                sp[k][HEADS ? j : 0][pos * TBR + t] = fmaf(qr[k][j][e], f[e], sp[k][HEADS ? j : 0][pos * TBR + t]);
                    }
                if constexpr (pos == NB - 1) {
#pragma unroll
                    for (int k = 0; k < TQ; ++k) {
                        if constexpr (HEADS) {
                            // complete the dot products inside each head's lane group (lg is wave-uniform)
                            heads_xor_step<NJ, 1>(sp[k]);
                            heads_xor_step<NJ, 2>(sp[k]);
                            if (lg > 2) heads_xor_step<NJ, 4>(sp[k]);
                            if (lg > 3) heads_xor_step<NJ, 8>(sp[k]);
                            if (lg > 4) heads_xor_step<NJ, 16>(sp[k]);
                            if (lg > 5) heads_xor_step<NJ, 32>(sp[k]);
#pragma unroll
                            for (int j = 0; j < NJ; ++j) {
                                float pm = -INFINITY;
#pragma unroll
                                for (int t = 0; t < 16; ++t) {
                                    sp[k][j][t] = div_by(sp[k][j][t], scale, inv_scale);
#if MLI_PROMPT_SOFTCAP
                                    sp[k][j][t] = softcap_score(sp[k][j][t], cap, inv_cap);
#endif
                                    pm = slot_live<true, true>(t, nt[k], nlo[k], nk) ? fmaxf(pm, sp[k][j][t]) : pm;
                                }
                                const float m_new = fmaxf(run_m[k][j], pm);
                                // (no live slot yet: m_new is -inf too, and the state stays empty)
                                const float alpha = run_m[k][j] == -INFINITY ? 0.f : expf(run_m[k][j] - m_new);
                                float psum = 0.f;
#pragma unroll
                                for (int t = 0; t < 16; ++t) {
                                    sp[k][j][t] = slot_live<true, true>(t, nt[k], nlo[k], nk) ? expf(sp[k][j][t] - m_new) : 0.f;
                                    psum += sp[k][j][t];
                                }
                                run_l[k][j] = run_l[k][j] * alpha + psum;
                                run_m[k][j] = m_new;
#pragma unroll
                                for (int e = 0; e < EPL; ++e) acc[k][j][e] *= alpha;
                            }
                        } else {
                            // all 16 slots scored: the lane holds the sum for slot (lane >> 2) & 15
                            const float tot = wave_reduce16(sp[k][0], lane);
                            const int slot = (lane >> 2) & 15;
                            const bool valid = slot_live<true, true>(slot, nt[k], nlo[k], nk);
                            const float score = tot / scale;
                            const float pm = wave_max(valid ? score : -INFINITY);
                            const float m_new = fmaxf(run_m[k][0], pm);
                            const float alpha = run_m[k][0] == -INFINITY ? 0.f : expf(run_m[k][0] - m_new);
                            p_lane[k] = valid ? expf(score - m_new) : 0.f;
                            run_l[k][0] = run_l[k][0] * alpha + wave_sum((lane & 3) == 0 ? p_lane[k] : 0.f);
                            run_m[k][0] = m_new;
#pragma unroll
                            for (int j = 0; j < NJ; ++j)
#pragma unroll
                                for (int e = 0; e < EPL; ++e) acc[k][j][e] *= alpha;
                        }
                    }
                }
            } else {
                // ---- V batch: acc[k] += p[k] . V over the slots live for query k ----
                constexpr int first_slot = (pos - NB) * TBR;
#pragma unroll
                for (int t = 0; t < TBR; ++t) {
                    float f[NJ][EPL];
#pragma unroll
                    for (int j = 0; j < NJ; ++j) E::unpack(buf[bi][t][j], f[j]);
#pragma unroll
                    for (int k = 0; k < TQ; ++k) {
                        // wave-uniform: never multiply a slot the query does not attend, even by zero
                        if (slot_live<true, true>(first_slot + t, nt[k], nlo[k], nk)) {
                            float p1 = 0.f;
                            if constexpr (!HEADS)   // the slot's probability sits in lane 4 * slot: broadcast through an SGPR
                                p1 = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(p_lane[k]), 4 * (first_slot + t)));
#pragma unroll
                            for (int j = 0; j < NJ; ++j) {
                                const float p = HEADS ? sp[k][HEADS ? j : 0][first_slot + t] : p1;
#pragma unroll
                                for (int e = 0; e < EPL; ++e) acc[k][j][e] = fmaf(p, f[j][e], acc[k][j][e]);
                            }
                        }
                    }
                }
            }
        });
        page = next;
    }

    // ---- the block's results, one query at a time: the waves (each owns whole pages) are merged in wave order through LDS ----
    static_for<TQ>([&](auto KQ) {
        constexpr int k = decltype(KQ)::value;
        if (k < nq) {   // workgroup-uniform
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                wave_ml[wave * kRowU + j * kWave + lane] = make_float2(run_m[k][HEADS ? j : 0], run_l[k][HEADS ? j : 0]);
#pragma unroll
                for (int e = 0; e < EPL; ++e) red[wave * kRowF + (j * kWave + lane) * EPL + e] = acc[k][j][e];
            }
            __syncthreads();
            float* o = out + (q_row0 + k) * D;
            // element i of the row lives at red[...][i]; the four elements of a thread share a lane unit, hence a head
            for (int i = 4 * threadIdx.x; i < D; i += 4 * kFuThreads) {
                const int u = i / EPL;
                float m = -INFINITY;
#pragma unroll
                for (int w = 0; w < kFuWaves; ++w) m = fmaxf(m, wave_ml[w * kRowU + u].x);
#if MLI_PROMPT_SINK_LOGITS
                // the query's final (m, l): the four elements of a thread share a head, hence z; the sink joins the maximum
                // before the waves' weights are formed
                const float zsink = sink_logits[i >> (lg + (EPL == 8 ? 3 : 2))];
                m = fmaxf(m, zsink);
#endif
                float wsc[kFuWaves];
                float l = 0.f;
#pragma unroll
                for (int w = 0; w < kFuWaves; ++w) {
                    const float2 s = wave_ml[w * kRowU + u];
                    wsc[w] = s.x == -INFINITY ? 0.f : expf(s.x - m);
                    l += s.y * wsc[w];
                }
#if MLI_PROMPT_SINK_LOGITS
                l += expf(zsink - m);   // the sink's share of the denominator; it has no value row
#endif
                const float norm = 1.f / l;
                float r[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    float t = 0.f;
#pragma unroll
                    for (int w = 0; w < kFuWaves; ++w) t += red[w * kRowF + i + c] * wsc[w];
                    r[c] = t * norm;
                }
                *reinterpret_cast<float4*>(o + i) = make_float4(r[0], r[1], r[2], r[3]);
            }
            __syncthreads();   // the next query parks into the same buffers
        }
    });
}
