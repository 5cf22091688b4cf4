// The tiled bf16-MFMA GEMM kernel of proj_gemm_bf16.hip, which includes this text twice: with MLI_GEMM_ROPE 0 it is
// gemm_bf16_mfma_kernel, with MLI_GEMM_ROPE 1 gemm_bf16_mfma_rope_kernel -- the same kernel with rotary position
// embeddings in its epilogue and the table as an argument of its own (GemmArgs keeps its layout).  One text, so the two
// cannot drift apart; two definitions, so the plain kernel's device code is what it was before the switch existed
// (tools/kernel_diff.py).  No include guard.
//
// MT = 32-row sub-tiles per wave (rows per workgroup = 64 * MT), KB = k extent of a staged tile (32 or 64)
// FP8 = the pages hold OCP e4m3 bytes (MLI_ELEM_FP8): A rows are widened to bf16 on their way into LDS (exact), K / V rows
// leave as fp8 (round to nearest even, saturating); the weights are bf16 and everything between is the bf16 kernel
// MODE_ = kPagedFillLive: kPagedFill over the live tokens (the windowed prefill), as in gemm_f32_mfma_kernel
// MLI_GEMM_ROPE: the epilogue rotates the K and q accumulators by the row's absolute slot before the one rounding to the
// page's element type (rope_rotate, gemm_common.hpp).  rope: [S][rope_half] (cos, sin) pairs, rope_half = hd / 2.
template <int MODE_, int MT = 1, int KB = 32, bool FP8 = false>
#if MLI_GEMM_ROPE
__global__ __launch_bounds__(kHThreads) void gemm_bf16_mfma_rope_kernel(GemmArgs g, const float2* __restrict__ rope, int rope_half) {
#else
__global__ __launch_bounds__(kHThreads) void gemm_bf16_mfma_kernel(GemmArgs g) {
#endif
    constexpr bool WIN = MODE_ == kPagedFillLive;   // the windowed prefill's fill: kPagedFill over the live tokens
    constexpr int MODE = WIN ? kPagedFill : MODE_;
    constexpr int HM = 64 * MT;              // shadows the namespace-level 64
    constexpr int HK = KB;
    constexpr int kLdaBytes = HK * 2 + 16;   // 80 / 144: ds_read_b128 fragment reads are conflict-free
    constexpr int AP = HM * HK / (kHThreads * 8);   // 16-byte A loads per thread and tile
    constexpr int BP = HK * HN / (kHThreads * 8);   // 16-byte B loads per thread and tile
    constexpr int kAThreadsPerRow = HK / 8;
    __shared__ __align__(16) unsigned char As[HM * kLdaBytes];
    __shared__ __align__(16) unsigned char Bs[HK * kLdbBytes];
    __shared__ const float* a_ptr[HM];
    __shared__ float* o_ptr[HM];
    constexpr bool kFillMode = MODE == kPagedFill;
    __shared__ const float* e_ptr[kFillMode ? HM : 1];  // embedding prologue: fp32 emb_table / wpe row of every A row
    __shared__ const float* p_ptr[kFillMode ? HM : 1];

    const int tiles_n = (g.N + HN - 1) / HN;
    const int wsel = blockIdx.x / tiles_n;
    const int n0 = (blockIdx.x % tiles_n) * HN;
    const int m0 = blockIdx.y * HM;
    const int z = blockIdx.z;
    const int out_id = g.out_id[wsel];
    const uint16_t* __restrict__ W = reinterpret_cast<const uint16_t*>(g.w[wsel]);

    constexpr bool kLatest = MODE == kPagedLatest;
    __shared__ FillIndex fill_index[1];
    const int tid = threadIdx.x;
    int fill_total = 0;
    if (g.compact) {
        fill_total = build_fill_index<kHThreads, kLatest, WIN>(g, fill_index[0]);
        if (m0 >= fill_total) return;  // workgroup-uniform: every lane leaves together
    } else if (MODE == kPagedFill && m0 >= g.lengths[g.new_batch_idx[z]]) {
        return;
    } else if (MODE == kPagedFill && WIN && fill_tile_dead(g, m0, HM, z)) {
        return;
    }
    const bool embed = kFillMode && g.emb_table != nullptr;
    if (tid < HM) {
        RowDesc r{nullptr, nullptr, nullptr, nullptr};
#if MLI_GEMM_ROPE
        int rm = m0 + tid;  // what resolve_row is given as m
#endif
        if (g.compact) {
            if (m0 + tid < fill_total) {
                int zz, ss;
                if (WIN) fill_index_lookup_live(g, fill_index[0], m0 + tid, zz, ss);
                else fill_index_lookup(fill_index[0], kLatest ? g.B : g.n_new, m0 + tid, zz, ss);
                r = kLatest ? resolve_row<MODE, true, FP8>(g, zz, 0, out_id) : resolve_row<MODE, true, FP8>(g, ss, zz, out_id);
#if MLI_GEMM_ROPE
                rm = kLatest ? zz : ss;
#endif
            }
        } else if (!WIN || !fill_token_dead(g, m0 + tid, z)) {
            r = resolve_row<MODE, true, FP8>(g, m0 + tid, z, out_id);
        }
        a_ptr[tid] = r.a;
        o_ptr[tid] = r.o;
#if MLI_GEMM_ROPE
        rope_slots<HM>()[tid] = rope_row_slot<kLatest>(g, rm);  // the row's absolute slot, beside o_ptr
#endif
        if (kFillMode) {
            e_ptr[tid] = r.e;
            p_ptr[tid] = r.p;
        }
    }
    __syncthreads();

    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = (wave >> 1) * 32 * MT;
    const int wn = (wave & 1) * 32;

    // staging coordinates: 16-byte loads, AP + BP per thread and tile
    const int a_row = tid / kAThreadsPerRow, a_k8 = (tid % kAThreadsPerRow) * 8;  // A: rows x chunks of 8 k
    constexpr int kARowsPerPass = kHThreads / kAThreadsPerRow;
    const int b_row = tid >> 3, b_n8 = (tid & 7) * 8;                            // B: 32 k-rows x 8 chunks of 8 n
    uint4 a_reg[AP], b_reg[BP];
    const uint16_t* a_src[AP];
    const float* e_src[AP];
    const float* p_src[AP];
#pragma unroll
    for (int p = 0; p < AP; ++p) {
        a_src[p] = reinterpret_cast<const uint16_t*>(a_ptr[a_row + p * kARowsPerPass]);
        e_src[p] = kFillMode ? e_ptr[a_row + p * kARowsPerPass] : nullptr;
        p_src[p] = kFillMode ? p_ptr[a_row + p * kARowsPerPass] : nullptr;
    }
    const bool writes_x = blockIdx.x == 0;  // first column tile of the first weight: every A element passes once

    auto load_tile = [&](int k0) {
#pragma unroll
        for (int p = 0; p < AP; ++p) {
            a_reg[p] = make_uint4(0, 0, 0, 0);
            if (kFillMode && embed && a_src[p] != nullptr) {
                // encoder as prologue: x = bf16(emb[tok] + wpe[s]) -- fp32 sum, one rounding, what the bf16 encoder
                // kernel writes -- fed to the MFMA and, by the first column tile, written to the page's segment 0
                if (k0 + a_k8 < g.K) {
                    const float4 e0 = *reinterpret_cast<const float4*>(e_src[p] + k0 + a_k8);
                    const float4 e1 = *reinterpret_cast<const float4*>(e_src[p] + k0 + a_k8 + 4);
                    const float4 p0 = *reinterpret_cast<const float4*>(p_src[p] + k0 + a_k8);
                    const float4 p1 = *reinterpret_cast<const float4*>(p_src[p] + k0 + a_k8 + 4);
                    if constexpr (FP8) {   // x = fp8(emb[tok] + wpe[s]): fp32 sum, one rounding; the MFMA sees what the page holds
                        const uint2 x8 = make_uint2(f32x4_to_fp8x4(e0.x + p0.x, e0.y + p0.y, e0.z + p0.z, e0.w + p0.w),
                                                    f32x4_to_fp8x4(e1.x + p1.x, e1.y + p1.y, e1.z + p1.z, e1.w + p1.w));
                        const uint2 lo = fp8x4_to_bf16x4(x8.x), hi = fp8x4_to_bf16x4(x8.y);
                        a_reg[p] = make_uint4(lo.x, lo.y, hi.x, hi.y);
                        if (writes_x)
                            *reinterpret_cast<uint2*>(const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(a_src[p])) + k0 + a_k8) = x8;
                    } else {
                        uint4 x;
                        x.x = f32_to_bf16(e0.x + p0.x) | ((uint32_t)f32_to_bf16(e0.y + p0.y) << 16);
                        x.y = f32_to_bf16(e0.z + p0.z) | ((uint32_t)f32_to_bf16(e0.w + p0.w) << 16);
                        x.z = f32_to_bf16(e1.x + p1.x) | ((uint32_t)f32_to_bf16(e1.y + p1.y) << 16);
                        x.w = f32_to_bf16(e1.z + p1.z) | ((uint32_t)f32_to_bf16(e1.w + p1.w) << 16);
                        a_reg[p] = x;
                        if (writes_x) *reinterpret_cast<uint4*>(const_cast<uint16_t*>(a_src[p]) + k0 + a_k8) = x;
                    }
                }
            } else if (a_src[p] != nullptr && k0 + a_k8 < g.K) {
                if constexpr (FP8) {   // 8 fp8 (8 bytes) -> 8 bf16
                    const uint2 x8 = *reinterpret_cast<const uint2*>(reinterpret_cast<const uint8_t*>(a_src[p]) + k0 + a_k8);
                    const uint2 lo = fp8x4_to_bf16x4(x8.x), hi = fp8x4_to_bf16x4(x8.y);
                    a_reg[p] = make_uint4(lo.x, lo.y, hi.x, hi.y);
                } else {
                    a_reg[p] = *reinterpret_cast<const uint4*>(a_src[p] + k0 + a_k8);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < BP; ++p) {
            b_reg[p] = make_uint4(0, 0, 0, 0);
            const int k = k0 + b_row + p * 32, n = n0 + b_n8;
            if (k < g.K && n < g.N) b_reg[p] = *reinterpret_cast<const uint4*>(W + (int64_t)k * g.N + n);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int p = 0; p < AP; ++p)
            *reinterpret_cast<uint4*>(&As[(a_row + p * kARowsPerPass) * kLdaBytes + a_k8 * 2]) = a_reg[p];
#pragma unroll
        for (int p = 0; p < BP; ++p)
            *reinterpret_cast<uint4*>(&Bs[(b_row + p * 32) * kLdbBytes + b_n8 * 2]) = b_reg[p];
    };

    f32x16_t acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[mt][i] = 0.f;

    // fragment addresses (constant over the k loop)
    const int li = lane & 31, lh = lane >> 5;
    const unsigned a_off = (unsigned)((wm + li) * kLdaBytes + lh * 16);
    // transposing read: lane 4q+p of a 16-lane group points at row q, columns 4p..4p+3 of the group's 4x16 block
    const int grp_col = wn + 16 * ((lane >> 4) & 1);
    const int tq = (lane >> 2) & 3, tp = lane & 3;
    const unsigned b_off = (unsigned)((8 * lh + tq) * kLdbBytes + (grp_col + 4 * tp) * 2);

    const int nk = (g.K + HK - 1) / HK;
#ifdef MLI_GEMM_TRACE
    unsigned long long gt_acc[5] = {0, 0, 0, 0, 0};
    const unsigned long long gt_begin = clock64();
#endif
    load_tile(0);
    store_tile();
    __syncthreads();
    for (int t = 0; t < nk; ++t) {
        MLI_GT(g0);
        if (t + 1 < nk) load_tile((t + 1) * HK);
        MLI_GT(g1);
        MLI_GT_ADD(0, g0, g1);
#pragma unroll
        for (int kk = 0; kk < HK; kk += 16) {
            Frag8 b;
            b.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(&Bs[b_off + kk * kLdbBytes]));
            b.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(&Bs[b_off + (kk + 4) * kLdbBytes]));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                Frag8 a;
                a.u = *reinterpret_cast<const uint4*>(&As[a_off + mt * 32 * kLdaBytes + kk * 2]);
                acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc[mt], 0, 0, 0);
            }
        }
        MLI_GT(g2);
        MLI_GT_ADD(1, g1, g2);
        __syncthreads();
        MLI_GT(g3);
        MLI_GT_ADD(2, g2, g3);
        if (t + 1 < nk) {
            store_tile();
            MLI_GT(g4);
            MLI_GT_ADD(3, g3, g4);
            __syncthreads();
            MLI_GT(g5);
            MLI_GT_ADD(4, g4, g5);
        }
    }
#ifdef MLI_GEMM_TRACE
    {
        const unsigned wg = blockIdx.x + gridDim.x * blockIdx.y;
        if (threadIdx.x == 0 && wg < (unsigned)kGemmTraceWgs) {
            for (int i = 0; i < 5; ++i) mli_gemm_trace[wg * 8 + i] = gt_acc[i];
            mli_gemm_trace[wg * 8 + 5] = clock64() - gt_begin;
            mli_gemm_trace[wg * 8 + 6] = gt_begin;
            mli_gemm_trace[wg * 8 + 7] = (unsigned long long)nk;
        }
    }
#endif

    // epilogue: register r of lane l is (row = (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), col = l & 31)
#if MLI_GEMM_ROPE
    const int rope_fi = ((n0 + wn + li) % (2 * rope_half)) >> 1;  // the pair's frequency index inside its head
#endif
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mi = wm + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
            const int n = n0 + wn + li;
            float* op = o_ptr[mi];
            float y = acc[mt][r];
#if MLI_GEMM_ROPE
            if (out_id <= 1) {  // (workgroup-uniform) K and q; the exchange comes before the guards
                const float other = rope_partner(y);
                if (op != nullptr && n < g.N)
                    y = rope_rotate(y, other, (li & 1) != 0, rope[(int64_t)rope_slots<HM>()[mi] * rope_half + rope_fi]);
            }
#endif
            if (op != nullptr && n < g.N) {
                if (out_id == 1) op[n] = y;                                         // q: fp32
                else if (FP8) reinterpret_cast<uint8_t*>(op)[n] = (uint8_t)f32_to_fp8(y);   // K / V: fp8 page rows
                else reinterpret_cast<uint16_t*>(op)[n] = f32_to_bf16(y);            // K / V: bf16 page rows
            }
        }
    }
}
