// The tiled fp32-MFMA GEMM kernel of proj_gemm.hip, which includes this text twice: with MLI_GEMM_ROPE 0 it is
// gemm_f32_mfma_kernel, with MLI_GEMM_ROPE 1 gemm_f32_mfma_rope_kernel -- the same kernel with rotary position embeddings
// in its epilogue and the table as an argument of its own (GemmArgs keeps its layout).  One text, so the two cannot drift
// apart; two definitions, so the plain kernel's device code is what it was before the switch existed
// (tools/kernel_diff.py).  No include guard.
//
// VEC4: K % 4 == 0, N % 4 == 0 and 16-byte aligned rows -> float4 global loads.
// BF16 (paged modes only): x, W and the K/V outputs are bfloat16, q and the accumulation fp32.  Operands are
// widened to fp32 while they are staged into LDS, so the product is still the exact fp32 MFMA chain
// (bf16 x bf16 products are exact in fp32); a native v_mfma_f32_32x32x16_bf16 tile is the next step.
// MT: 32-row sub-tiles per wave along M.  MT = 2 (128x64 workgroup tile) shares every weight fragment between two
// MFMAs with independent accumulators: 1.5 instead of 2 LDS fragment reads per MFMA and half the barriers per flop.
// KQ: 32-deep k slabs staged per tile.  Only KQ = 1 is instantiated: 128 k per barrier pair (KQ = 4) was measured
// SLOWER for the latency-bound fp32 shapes (config 4 logits 23.8 -> 26.0 us, D = 2048 logits 61.8 -> 70.2 us) --
// unlike the bf16 kernel, whose deep tile is a win (proj_gemm_bf16.hip).
// MODE_ = kPagedFillLive (launched by the windowed prefill only) is kPagedFill with WIN set: the fill of a row's live tokens
// under a sliding window with sinks (gemm_common.hpp, page_live.hpp).
// MLI_GEMM_ROPE (the paged modes, not transposed): the epilogue rotates the K and q accumulators by the row's absolute slot
// before the one rounding (rope_rotate, gemm_common.hpp).  rope: [S][rope_half] (cos, sin) pairs, rope_half = hd / 2.
template <int MODE_, bool BT, bool VEC4, bool BF16 = false, int MT = 1, bool SPLIT = false>
#if MLI_GEMM_ROPE
__global__ __launch_bounds__(SPLIT ? 2 * kGemmThreads : kGemmThreads) void gemm_f32_mfma_rope_kernel(GemmArgs g, const float2* __restrict__ rope,
                                                                                                      int rope_half) {
    static_assert(!BT && (MODE_ == kPagedLatest || MODE_ == kPagedFill || MODE_ == kPagedFillLive), "paged modes only");
#else
__global__ __launch_bounds__(SPLIT ? 2 * kGemmThreads : kGemmThreads) void gemm_f32_mfma_kernel(GemmArgs g) {
#endif
    constexpr bool WIN = MODE_ == kPagedFillLive;   // the windowed prefill's fill: kPagedFill over the live tokens
    constexpr int MODE = WIN ? kPagedFill : MODE_;
    constexpr int BM = 64 * MT;   // shadows the namespace-level 64: rows per workgroup
    constexpr int BK = 32;        // k extent of a staged tile
    constexpr int KQ = 1;
    constexpr int LDA = BM + 1;
    constexpr int kBufs = SPLIT ? 2 : 1;
    constexpr int kThreads = SPLIT ? 2 * kGemmThreads : kGemmThreads;
    __shared__ float As[kBufs * BK * LDA];
    constexpr int LDBX = BT ? LDBT : LDB;
    __shared__ __align__(16) float Bs[kBufs * BK * LDBX];
    __shared__ const float* a_ptr[BM];
    __shared__ float* o_ptr[BM];
    constexpr bool kFillMode = MODE == kNaiveFill || MODE == kPagedFill;
    __shared__ const float* e_ptr[kFillMode ? BM : 1];  // embedding prologue: emb_table / wpe row of every A row
    __shared__ const float* p_ptr[kFillMode ? BM : 1];

    const int tiles_n = (g.N + BN - 1) / BN;
    const int wsel = blockIdx.x / tiles_n;
    const int n0 = (blockIdx.x % tiles_n) * BN;
    const int m0 = blockIdx.y * BM;
    const int z = blockIdx.z;
    const int out_id = g.out_id[wsel];
    const float* __restrict__ Bmat = g.w[wsel];

    constexpr bool kFill = MODE == kNaiveFill || MODE == kPagedFill;
    constexpr bool kLatest = MODE == kNaiveLatest || MODE == kPagedLatest;
    __shared__ std::conditional_t<kFill || kLatest, FillIndex, NoFillIndex> fill_index[1];
    const int tid = threadIdx.x;
    int fill_total = 0;
    if (kFill || kLatest) {
        if (g.compact) {
            fill_total = build_fill_index<kThreads, kLatest, WIN>(g, fill_index[0]);
            if (m0 >= fill_total) return;  // workgroup-uniform
        } else if (kFill && m0 >= g.lengths[g.new_batch_idx[z]]) {
            return;  // whole tile beyond the row's length: nothing to do (reference …optimized.cu:43-45)
        } else if (kFill && WIN && fill_tile_dead(g, m0, BM, z)) {
            return;  // ... or wholly in dead pages
        }
    }

    const bool embed = kFillMode && !BF16 && g.emb_table != nullptr;
    if (tid < BM) {  // BM <= 128 < 256 threads
        RowDesc r{nullptr, nullptr, nullptr, nullptr};
#if MLI_GEMM_ROPE
        int rm = m0 + tid;  // what resolve_row is given as m
#endif
        if ((kFill || kLatest) && g.compact) {
            if (m0 + tid < fill_total) {
                int zz, ss;
                if (WIN) fill_index_lookup_live(g, fill_index[0], m0 + tid, zz, ss);
                else fill_index_lookup(fill_index[0], kLatest ? g.B : g.n_new, m0 + tid, zz, ss);
                r = kLatest ? resolve_row<MODE, BF16>(g, zz, 0, out_id) : resolve_row<MODE, BF16>(g, ss, zz, out_id);
#if MLI_GEMM_ROPE
                rm = kLatest ? zz : ss;
#endif
            }
        } else if (!WIN || !fill_token_dead(g, m0 + tid, z)) {
            r = resolve_row<MODE, BF16>(g, m0 + tid, z, out_id);
        }
        a_ptr[tid] = r.a;
        o_ptr[tid] = r.o;
#if MLI_GEMM_ROPE
        rope_slots<BM>()[tid] = rope_row_slot<kLatest>(g, rm);  // the row's absolute slot, beside o_ptr
#endif
        if (kFillMode) {
            e_ptr[tid] = r.e;
            p_ptr[tid] = r.p;
        }
    }
    // only the contiguous layout keeps K transposed (kt_cache[b, n, s]): element stride S along n
    constexpr bool kCanTranspose = MODE == kNaiveLatest || MODE == kNaiveFill;
    const bool transposed_out = kCanTranspose && out_id == 0;
    const int64_t o_stride = transposed_out ? g.S : 1;
    __syncthreads();

    // SPLIT: threads 0..255 (waves 0-3) multiply, threads 256..511 (waves 4-7) move the next tile into the other LDS buffer
    const bool is_loader = SPLIT && tid >= kGemmThreads;
    const int st = is_loader ? tid - kGemmThreads : tid;   // index among the staging threads
    const int lane = tid & 63;
    const int wave = (tid >> 6) & 3;
    const int wm = (wave >> 1) * 32 * MT;
    const int wn = (wave & 1) * 32;

    // global -> register staging coordinates
    //   A tile [BM][BK]: 8 threads per row (float4 along k), 32 rows per pass, 2 passes
    //   B tile [BK][BN]: 16 threads per k-row (float4 along n), 16 k-rows per pass, 2 passes
    //   B^T tile (BT): rows are n, float4 along k -- same shape as the A tile
    const int a_row = st >> 3, a_kq = (st & 7) * 4;
    const int b_row = st >> 4, b_nq = (st & 15) * 4;
    constexpr int AP = 2 * MT;  // A staging passes of 32 rows
    float4 a_regs[KQ][AP], b_regs[KQ][2];
    // this thread's source rows, kept in registers: re-reading them from LDS every tile put a wait-for-LDS and a
    // branch per pass into every k step
    const float* a_src[AP];
    const float* e_src[AP];
    const float* p_src[AP];
#pragma unroll
    for (int p = 0; p < AP; ++p) {
        a_src[p] = a_ptr[a_row + p * 32];
        e_src[p] = kFillMode ? e_ptr[a_row + p * 32] : nullptr;
        p_src[p] = kFillMode ? p_ptr[a_row + p * 32] : nullptr;
    }
    const bool writes_x = blockIdx.x == 0;  // first column tile of the first weight: every A element passes once

    auto load_slab = [&](int k0, float4 (&a_reg)[AP], float4 (&b_reg)[2]) {
#pragma unroll
        for (int p = 0; p < AP; ++p) {
            const float* ap = a_src[p];
            const int k = k0 + a_kq;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (kFillMode && embed && ap != nullptr) {
                // encoder as prologue: x = emb[tok] + wpe[s], the sum the encoder kernel writes (one fp32 add)
                if (VEC4) {
                    if (k < g.K) {
                        const float4 e4 = *reinterpret_cast<const float4*>(e_src[p] + k);
                        const float4 p4 = *reinterpret_cast<const float4*>(p_src[p] + k);
                        v = make_float4(e4.x + p4.x, e4.y + p4.y, e4.z + p4.z, e4.w + p4.w);
                        if (writes_x) *reinterpret_cast<float4*>(const_cast<float*>(ap) + k) = v;
                    }
                } else {
                    float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int i = 0; i < 4; ++i)
                        if (k + i < g.K) {
                            t[i] = e_src[p][k + i] + p_src[p][k + i];
                            if (writes_x) const_cast<float*>(ap)[k + i] = t[i];
                        }
                    v = make_float4(t[0], t[1], t[2], t[3]);
                }
            } else if (ap != nullptr) {
                if (BF16) {
                    if (k < g.K) v = load4_bf16(reinterpret_cast<const uint16_t*>(ap) + k);
                } else if (VEC4) {
                    if (k < g.K) v = *reinterpret_cast<const float4*>(ap + k);
                } else {
                    if (k + 0 < g.K) v.x = ap[k + 0];
                    if (k + 1 < g.K) v.y = ap[k + 1];
                    if (k + 2 < g.K) v.z = ap[k + 2];
                    if (k + 3 < g.K) v.w = ap[k + 3];
                }
            }
            a_reg[p] = v;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (BT) {
                const int n = n0 + a_row + p * 32;
                const int k = k0 + a_kq;
                if (n < g.N) {
                    const float* bp = Bmat + (int64_t)n * g.K + k;
                    if (VEC4) {
                        if (k < g.K) v = *reinterpret_cast<const float4*>(bp);
                    } else {
                        if (k + 0 < g.K) v.x = bp[0];
                        if (k + 1 < g.K) v.y = bp[1];
                        if (k + 2 < g.K) v.z = bp[2];
                        if (k + 3 < g.K) v.w = bp[3];
                    }
                }
            } else {
                const int k = k0 + b_row + p * 16;
                const int n = n0 + b_nq;
                if (k < g.K) {
                    const float* bp = Bmat + (int64_t)k * g.N + n;
                    if (BF16) {
                        if (n < g.N) v = load4_bf16(reinterpret_cast<const uint16_t*>(Bmat) + (int64_t)k * g.N + n);
                    } else if (VEC4) {
                        if (n < g.N) v = *reinterpret_cast<const float4*>(bp);
                    } else {
                        if (n + 0 < g.N) v.x = bp[0];
                        if (n + 1 < g.N) v.y = bp[1];
                        if (n + 2 < g.N) v.z = bp[2];
                        if (n + 3 < g.N) v.w = bp[3];
                    }
                }
            }
            b_reg[p] = v;
        }
    };
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int q = 0; q < KQ; ++q) load_slab(k0 + q * 32, a_regs[q], b_regs[q]);
    };

    auto store_slab = [&](float* As_q, float* Bs_q, const float4 (&a_reg)[AP], const float4 (&b_reg)[2]) {
#pragma unroll
        for (int p = 0; p < AP; ++p) {
            const int m = a_row + p * 32;
            As_q[(a_kq + 0) * LDA + m] = a_reg[p].x;
            As_q[(a_kq + 1) * LDA + m] = a_reg[p].y;
            As_q[(a_kq + 2) * LDA + m] = a_reg[p].z;
            As_q[(a_kq + 3) * LDA + m] = a_reg[p].w;
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (BT) {
                const int n = a_row + p * 32;
                Bs_q[(a_kq + 0) * LDBX + n] = b_reg[p].x;
                Bs_q[(a_kq + 1) * LDBX + n] = b_reg[p].y;
                Bs_q[(a_kq + 2) * LDBX + n] = b_reg[p].z;
                Bs_q[(a_kq + 3) * LDBX + n] = b_reg[p].w;
            } else {
                *reinterpret_cast<float4*>(&Bs_q[(b_row + p * 16) * LDBX + b_nq]) = b_reg[p];
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int q = 0; q < KQ; ++q) store_slab(As + q * 32 * LDA, Bs + q * 32 * LDBX, a_regs[q], b_regs[q]);
    };

    f32x16 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

    const int nk = (g.K + BK - 1) / BK;
    const int lk = lane >> 5;   // which of the 2 k's of an MFMA step this lane feeds
    const int li = lane & 31;   // row (A) / column (B) inside the 32x32 wave tile

    auto multiply = [&](const float* A, const float* B) {
#pragma unroll
        for (int kk = 0; kk < BK; kk += 2) {
            const float b = B[(kk + lk) * LDBX + wn + li];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const float a = A[(kk + lk) * LDA + wm + mt * 32 + li];
                // the K output of the contiguous layout is stored transposed: swap operands so
                // that the sequence index lands on the lane (coalesced kt_cache stores)
                if (transposed_out) acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(b, a, acc[mt], 0, 0, 0);
                else acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[mt], 0, 0, 0);
            }
        }
    };
    if constexpr (!SPLIT) {
        load_tile(0);
        store_tile();
        __syncthreads();
        for (int t = 0; t < nk; ++t) {
            if (t + 1 < nk) load_tile((t + 1) * BK);  // in flight under the MFMAs below
            multiply(As, Bs);
            __syncthreads();
            if (t + 1 < nk) {
                store_tile();
                __syncthreads();
            }
        }
    } else {
        // One wave doing everything in turn (issue loads, wait, write LDS, read fragments, multiply) is overlapped only by
        // the other waves of its SIMD; with about one workgroup per CU (logits of 1024 rows, prefill of a few hundred
        // tokens: 256 tiles of 64 x 64) nothing overlaps and the matrix pipe idles half the time.  Here four waves only load
        // (two tiles in flight in their registers) and four only multiply, one barrier per k step -- the structure round 2
        // found on the bf16 projection (whose loaders have since become LDS-DMA issuers, proj_gemm_bf16.hip).  Same MFMA
        // chain per output element: bit-identical results.
        float* As1 = As + BK * LDA;
        float* Bs1 = Bs + BK * LDBX;
        if (is_loader) {
            float4 a2[AP], b2[2];
            load_slab(0, a_regs[0], b_regs[0]);
            if (1 < nk) load_slab(BK, a2, b2);
            store_slab(As, Bs, a_regs[0], b_regs[0]);
            if (2 < nk) load_slab(2 * BK, a_regs[0], b_regs[0]);
            __syncthreads();  // tile 0 is in buffer 0
            for (int t = 0; t < nk; t += 2) {
                if (t + 1 < nk) store_slab(As1, Bs1, a2, b2);                       // tile t + 1
                if (t + 3 < nk) load_slab((t + 3) * BK, a2, b2);
                __syncthreads();
                if (t + 1 < nk) {
                    if (t + 2 < nk) store_slab(As, Bs, a_regs[0], b_regs[0]);      // tile t + 2
                    if (t + 4 < nk) load_slab((t + 4) * BK, a_regs[0], b_regs[0]);
                    __syncthreads();
                }
            }
        } else {
            __syncthreads();  // tile 0 is in buffer 0
            for (int t = 0; t < nk; t += 2) {
                multiply(As, Bs);
                __syncthreads();
                if (t + 1 < nk) {
                    multiply(As1, Bs1);
                    __syncthreads();
                }
            }
        }
    }

    // epilogue: accumulator register r of lane l is tile element
    //   (row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col = l & 31)
    if (MODE == kPlain && g.row_best != nullptr) {
        // argmax epilogue (decoder logits): a row of the wave's 32x32 sub-tile lies across 32 lanes of one register
        // -> butterfly over the 5 low lane bits; the two waves that share the rows meet in LDS (the staging tiles are
        // free after the k loop's last barrier); one (max, index) pair per (row, column tile) goes to memory
        float* best_v = As;                                   // [BM][2]
        int* best_i = reinterpret_cast<int*>(As + BM * 2);    // [BM][2]   (BK * LDA >= 4 * BM floats)
        const int n = n0 + wn + li;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (is_loader) break;  // (wave-uniform: the loader waves only meet the barrier below)
            // a score takes part only if it beats -FLT_MAX, as in decoder_argmax_kernel (NaN and -inf never win)
            float v[16];
            int ix[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const bool takes_part = n < g.N && acc[mt][r] > -3.402823466e+38f;
                v[r] = takes_part ? acc[mt][r] : -3.402823466e+38f;
                ix[r] = takes_part ? n : -1;
            }
            // Transposing butterfly over the 32 lanes that hold one row per register: at every step a lane keeps half
            // of its rows and trades the other half with its partner (15 exchanges instead of 16 x 5), branch-free,
            // so the exchanges of different rows overlap.  Afterwards lane li holds row register (li >> 1) & 15.
            argmax_butterfly_step<8>(v, ix, (lane & 16) != 0, 16);
            argmax_butterfly_step<4>(v, ix, (lane & 8) != 0, 8);
            argmax_butterfly_step<2>(v, ix, (lane & 4) != 0, 4);
            argmax_butterfly_step<1>(v, ix, (lane & 2) != 0, 2);
            {
                const float ov = __shfl_xor(v[0], 1, kWave);
                const int oi = __shfl_xor(ix[0], 1, kWave);
                argmax_take(v[0], ix[0], ov, oi);
            }
            if ((li & 1) == 0) {
                const int r = (li >> 1) & 15;
                const int row = wm + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                best_v[row * 2 + (wave & 1)] = v[0];
                best_i[row * 2 + (wave & 1)] = ix[0];
            }
        }
        __syncthreads();
        if (!is_loader && tid < BM && m0 + tid < g.M) {
            float v = best_v[tid * 2];
            int i = best_i[tid * 2];
            argmax_take(v, i, best_v[tid * 2 + 1], best_i[tid * 2 + 1]);
            g.row_best[(int64_t)(m0 + tid) * tiles_n + blockIdx.x % tiles_n] = RowBest{v, i};
        }
        return;
    }
    if (is_loader) return;
#if MLI_GEMM_ROPE
    const int rope_fi = ((n0 + wn + li) % (2 * rope_half)) >> 1;  // the pair's frequency index inside its head
#endif
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int trow = (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (transposed_out) {
                const int n = n0 + wn + trow;   // rows of the swapped product run along N
                const int mi = wm + mt * 32 + li;
                float* op = o_ptr[mi];
                if (op != nullptr && n < g.N) op[(int64_t)n * o_stride] = acc[mt][r];
            } else {
                const int mi = wm + mt * 32 + trow;
                const int n = n0 + wn + li;
                float* op = o_ptr[mi];
                float y = acc[mt][r];
#if MLI_GEMM_ROPE
                if (out_id <= 1) {  // (workgroup-uniform) K and q; the exchange comes before the guards
                    const float other = rope_partner(y);
                    if (op != nullptr && n < g.N)
                        y = rope_rotate(y, other, (li & 1) != 0, rope[(int64_t)rope_slots<BM>()[mi] * rope_half + rope_fi]);
                }
#endif
                if (op != nullptr && n < g.N) {
                    if (BF16 && out_id != 1) reinterpret_cast<uint16_t*>(op)[n] = f32_to_bf16(y);
                    else op[n] = y;
                }
            }
        }
    }
}
