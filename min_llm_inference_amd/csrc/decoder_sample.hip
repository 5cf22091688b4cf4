// Sampled decoder head: a seeded temperature / top-k / top-p draw per batch row from materialised logits,
// then exactly what the greedy heads do with the token (result, length update, next input embedding).
//
// Per row b (logits x[0..V), position L = lengths[b], parameters T, K, P, seed):
//   T == 0        the greedy token: larger value, then lower index, only values above -FLT_MAX (decoder_argmax_kernel)
//   candidates    the finite x[v]
//   top-k         keep x[v] >= t_k, the K-th largest candidate (ties at t_k kept); K == 0 or K >= #candidates keeps all
//   top-p         keep x[v] >= t_p, the largest kept t whose softmax(x / T) mass over kept x[u] >= t is at least P
//   draw          argmax over the kept set of x[v] / T + g(seed, L, v), ties to the lower index, where
//                 g = -log(-log(u)), u = ((w >> 9) + 0.5f) * 2^-23, w = Philox4x32-10((v >> 2, L, 0, 0), seed)[v & 3]
// Out-of-domain device values: T < 0 or NaN = greedy; K < 0 = 0; P > 1 or NaN = 1; P <= 0 keeps only the largest value.
//
// One 256-thread workgroup per row, nothing depends on the row index beyond addressing.  The row's logits are staged in
// LDS when they fit kStageMax, otherwise every pass re-reads them from global memory (L2).  Thresholds are searched on the
// order-preserving uint32 key of the float, 15 probes per pass (a 16-ary search: <= 8 passes for 32 bits).  A probe's
// weight -- 1 for the top-k count, exp(x / T - max / T) for the top-p mass -- is summed per thread in stride order and
// reduced by a fixed butterfly and a fixed cross-wave order: no atomics, the result depends on the row's data and V only.
//
// Log-probabilities (the LOGPROBS instantiations): after the pick the same workgroup reports, for the RAW
// distribution of the row (no temperature, top-k or top-p: greedy and sampled rows on one scale),
//   logprob(v) = (x_v - m) - log(sum over candidates of exp(x_u - m)),  m = the largest candidate
// of the emitted token and of the n_top <= 8 candidates of largest logit, ordered by (logit descending, index ascending).
// The alternatives are selected in one pass -- every thread keeps the 8 best of its own candidates in registers -- and
// n_top rounds of block_argmax over the heads of those lists: comparisons only, no marks in the row, no scratch.  expf /
// logf, the sum per thread in stride order and block_sum's fixed order: the figures depend on the row's data and V only.
// Without the switch the kernels are the ones they were.
#include <cfloat>

#include "embed_store.hpp"

namespace mli {

int launch_gemm_nt(const float* A, const float* Bt, float* C, int M, int N, int K, hipStream_t st);

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kProbes = 15;          // thresholds per pass of the threshold search
constexpr int kStageMax = 15 * 1024;  // logits staged in LDS up to this many per row (60 KiB, under the 64 KiB default)

struct SampleShared {
    float red[kWaves][kProbes];
    uint32_t kmax[kWaves], kmin[kWaves];
    float bv[kWaves];
    int bi[kWaves];
};

// Philox4x32-10 (Salmon et al., SC'11): multipliers D2511F53 / CD9E8D57, Weyl key increments 9E3779B9 / BB67AE85
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
        }
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
    }
    return c;
}

// Gumbel noise of one 32-bit draw.  u = the midpoint of one of 2^23 equal bins, exact in fp32 and strictly inside (0, 1):
// with 24 bits, ((w >> 8) + 0.5f) rounds to 2^24 for the top bin (u = 1, g = +inf: that entry would always win)
__device__ __forceinline__ float gumbel(uint32_t w) {
    const float u = __fmul_rn(__fadd_rn((float)(w >> 9), 0.5f), 1.1920928955078125e-07f);  // 2^-23
    return -logf(-logf(u));
}

__device__ __forceinline__ bool finite_bits(float f) { return (__float_as_uint(f) & 0x7f800000u) != 0x7f800000u; }

// order-preserving key: a < b  <=>  key(a) < key(b) for finite floats; -0 and +0 share the key of +0
__device__ __forceinline__ uint32_t order_key(float f) {
    uint32_t u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// sum of a[] over the workgroup, in a fixed order; every thread gets the sums
template <int N>
__device__ __forceinline__ void block_sum(float (&a)[N], SampleShared& sh) {
#pragma unroll
    for (int k = 0; k < N; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) a[k] += __shfl_xor(a[k], off, kWave);
    __syncthreads();  // earlier readers of sh.red are done
    if ((threadIdx.x & (kWave - 1)) == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) sh.red[threadIdx.x / kWave][k] = a[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float s = sh.red[0][k];
        for (int w = 1; w < kWaves; ++w) s += sh.red[w][k];
        a[k] = s;
    }
}

// (value, index) argmax over the workgroup: larger value, then lower index (argmax_take); every thread gets the index
__device__ __forceinline__ int block_argmax(float mv, int mi, SampleShared& sh) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(mv, off, kWave);
        const int oi = __shfl_xor(mi, off, kWave);
        argmax_take(mv, mi, ov, oi);
    }
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sh.bv[threadIdx.x / kWave] = mv;
        sh.bi[threadIdx.x / kWave] = mi;
    }
    __syncthreads();
    float bv = sh.bv[0];
    int bi = sh.bi[0];
    for (int w = 1; w < kWaves; ++w) argmax_take(bv, bi, sh.bv[w], sh.bi[w]);
    return bi;
}

// f(p) = sum over candidates with key >= p of (MASS ? exp(x / T - zmax) : 1), for N probes p[] >= lo at once
template <int N, bool MASS>
__device__ __forceinline__ void probe_sums(const float* x, int V, uint32_t lo, const uint32_t (&p)[N], float T, float zmax,
                                           float (&acc)[N], SampleShared& sh) {
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = 0.f;
    for (int v = threadIdx.x; v < V; v += kThreads) {
        const float xv = x[v];
        if (!finite_bits(xv)) continue;
        const uint32_t key = order_key(xv);
        if (key < lo) continue;
        const float w = MASS ? expf(__fsub_rn(__fdiv_rn(xv, T), zmax)) : 1.f;
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] += key >= p[k] ? w : 0.f;
    }
    block_sum(acc, sh);
}

// The largest key t in [lo, hi] with f(t) >= target, given f(lo) >= target (f is non-increasing).  16-ary search: each
// pass probes 15 keys spread over the range and keeps the sub-range after the last one that still qualifies.  lo / hi
// and every sum are the same in all threads, so the loop is uniform.
template <bool MASS>
__device__ __forceinline__ uint32_t search_threshold(const float* x, int V, uint32_t lo, uint32_t hi, float target, float T, float zmax,
                                     SampleShared& sh) {
    while (lo < hi) {
        const uint64_t span = (uint64_t)(hi - lo) + 1;
        uint32_t p[kProbes];
#pragma unroll
        for (int k = 0; k < kProbes; ++k) p[k] = lo + (uint32_t)(((uint64_t)(k + 1) * span) >> 4);  // lo <= p[k] <= hi
        float f[kProbes];
        probe_sums<kProbes, MASS>(x, V, lo, p, T, zmax, f, sh);
        int j = 0;  // number of probes that qualify (a prefix, f being non-increasing)
#pragma unroll
        for (int k = 0; k < kProbes; ++k)
            if (f[k] >= target) j = k + 1;
        if (j < kProbes) hi = p[j] - 1;  // p[j] fails, so p[j] > lo
        if (j > 0) lo = p[j - 1];
    }
    return lo;
}

// Where the LOGPROBS kernels report (the arrays of mli_sample_tokens_logprobs); nothing without the switch
template <bool LOGPROBS>
struct LogprobOut {};
template <>
struct LogprobOut<true> {
    float* token_logprob;  // [rows]
    int* top_ids;          // [rows, n_top]
    float* top_logprobs;   // [rows, n_top]
    int n_top;
};

// a row that emits no token: -inf, ids -1, logprobs -inf
__device__ __forceinline__ void no_token_logprobs(const LogprobOut<true>& o, int64_t slot) {
    if (threadIdx.x == 0) o.token_logprob[slot] = -INFINITY;
    for (int k = threadIdx.x; k < o.n_top; k += kThreads) {
        o.top_ids[slot * o.n_top + k] = -1;
        o.top_logprobs[slot * o.n_top + k] = -INFINITY;
    }
}

// The figures of one row after its pick.  x = the row (staged or global), tok = the emitted token (every thread has it).
__device__ __forceinline__ void row_logprobs(const float* x, int V, int tok, const LogprobOut<true>& o, int64_t slot,
                                             SampleShared& sh) {
    if (tok < 0) {  // no candidate
        no_token_logprobs(o, slot);
        return;
    }
    // One pass: every thread keeps the kTop best of its own candidates, sorted by (value descending, index ascending) --
    // it meets them by ascending index, so an equal value goes behind.  Static indices only: the lists live in registers.
    constexpr int kTop = MLI_MAX_TOP_LOGPROBS;
    float tv[kTop];
    int ti[kTop];
#pragma unroll
    for (int j = 0; j < kTop; ++j) {
        tv[j] = -INFINITY;
        ti[j] = -1;
    }
    for (int v = threadIdx.x; v < V; v += kThreads) {
        const float xv = x[v];
        if (!finite_bits(xv) || !(xv > tv[kTop - 1])) continue;
        tv[kTop - 1] = xv;
        ti[kTop - 1] = v;
#pragma unroll
        for (int j = kTop - 1; j > 0; --j) {
            const bool up = tv[j] > tv[j - 1];
            const float fv = tv[j];
            const int fi = ti[j];
            tv[j] = up ? tv[j - 1] : fv;
            ti[j] = up ? ti[j - 1] : fi;
            tv[j - 1] = up ? fv : tv[j - 1];
            ti[j - 1] = up ? fi : ti[j - 1];
        }
    }
    // Then n_top rounds over the lists' heads: the next alternative overall is the head of some thread's list, and the
    // thread that owns the winner moves on to its next (no thread gives more than n_top <= kTop).
    float m = 0.f, log_s = 0.f;
    int n_found = 0;
    const int rounds = max(o.n_top, 1);  // the first round finds m, needed without alternatives too
    for (int k = 0; k < rounds; ++k) {
        const int bi = block_argmax(tv[0], ti[0], sh);
        if (bi < 0) break;  // fewer candidates than n_top (the same in every thread)
        const float pv = x[bi];
        if (ti[0] == bi) {
#pragma unroll
            for (int j = 0; j + 1 < kTop; ++j) {
                tv[j] = tv[j + 1];
                ti[j] = ti[j + 1];
            }
            tv[kTop - 1] = -INFINITY;
            ti[kTop - 1] = -1;
        }
        if (k == 0) {
            m = pv;
            float s[1] = {0.f};
            for (int v = threadIdx.x; v < V; v += kThreads) {
                const float xv = x[v];
                if (finite_bits(xv)) s[0] += expf(__fsub_rn(xv, m));
            }
            block_sum(s, sh);
            log_s = logf(s[0]);
        }
        if (k < o.n_top && threadIdx.x == 0) {
            o.top_ids[slot * o.n_top + k] = bi;
            o.top_logprobs[slot * o.n_top + k] = __fsub_rn(__fsub_rn(pv, m), log_s);
        }
        n_found = k + 1;
    }
    for (int k = n_found + threadIdx.x; k < o.n_top; k += kThreads) {
        o.top_ids[slot * o.n_top + k] = -1;
        o.top_logprobs[slot * o.n_top + k] = -INFINITY;
    }
    if (threadIdx.x == 0) {
        const float xt = x[tok];
        // a candidate (then n_found >= 1), or a token the greedy head took for its +inf; -inf and NaN are never taken
        o.token_logprob[slot] = finite_bits(xt) && n_found > 0 ? __fsub_rn(__fsub_rn(xt, m), log_s)
                                                                : (xt == -INFINITY ? -INFINITY : NAN);
    }
}

// The drawn token of one row with T > 0 (every thread returns it).  x = the row's logits, staged or global.
__device__ __forceinline__ int draw_row(const float* x, int V, float T, int K, float P, uint64_t seed, int L, SampleShared& sh) {
    // candidates: count and key range
    float n_cand[1] = {0.f};  // exact: V < 2^24
    uint32_t kmax = 0u, kmin = 0xffffffffu;
    for (int v = threadIdx.x; v < V; v += kThreads) {
        const float xv = x[v];
        if (!finite_bits(xv)) continue;
        const uint32_t key = order_key(xv);
        n_cand[0] += 1.f;
        kmax = max(kmax, key);
        kmin = min(kmin, key);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kmax = max(kmax, (uint32_t)__shfl_xor((int)kmax, off, kWave));
        kmin = min(kmin, (uint32_t)__shfl_xor((int)kmin, off, kWave));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
        sh.kmax[threadIdx.x / kWave] = kmax;
        sh.kmin[threadIdx.x / kWave] = kmin;
    }
    block_sum(n_cand, sh);  // its barriers also publish kmax / kmin
    for (int w = 0; w < kWaves; ++w) {
        kmax = max(kmax, sh.kmax[w]);
        kmin = min(kmin, sh.kmin[w]);
    }
    if (n_cand[0] == 0.f) return -1;  // nothing takes part: the greedy head's answer

    uint32_t lo = kmin;  // kept set = candidates with key >= lo
    const float zmax = __fdiv_rn(key_value(kmax), T);
    if (K > 0 && (float)K < n_cand[0]) lo = search_threshold<false>(x, V, lo, kmax, (float)K, T, zmax, sh);
    if (P < 1.f) {  // NaN compares false: no top-p
        const uint32_t at_lo[1] = {lo};
        float total[1];
        probe_sums<1, true>(x, V, lo, at_lo, T, zmax, total, sh);
        lo = search_threshold<true>(x, V, lo, kmax, P * total[0], T, zmax, sh);
    }

    // Gumbel-max over the kept set: one Philox call per 4 consecutive vocabulary entries
    const uint32_t s_lo = (uint32_t)seed, s_hi = (uint32_t)(seed >> 32);
    float mv = -INFINITY;
    int mi = -1;
    for (int q = threadIdx.x; 4 * q < V; q += kThreads) {
        const uint4 r = philox4x32_10(make_uint4((uint32_t)q, (uint32_t)L, 0u, 0u), s_lo, s_hi);
        const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int v = 4 * q + j;
            if (v >= V) break;
            const float xv = x[v];
            if (!finite_bits(xv) || order_key(xv) < lo) continue;
            argmax_take(mv, mi, __fadd_rn(__fdiv_rn(xv, T), gumbel(w[j])), v);
        }
    }
    return block_argmax(mv, mi, sh);
}

// The token of one row (every thread returns it).  xg = the row's logits in global memory; stage = dynamic LDS of
// min(V, kStageMax) floats when V <= kStageMax.  LOGPROBS: the row's figures are reported too (slot = its place in the
// output arrays), and a greedy row is staged as well -- its token comes from the same values in the same order.
template <bool LOGPROBS>
__device__ __forceinline__ int sample_row(const float* __restrict__ xg, int V, float T, int K, float P, uint64_t seed, int L,
                                          float* stage, SampleShared& sh, const LogprobOut<LOGPROBS>& out, int64_t slot) {
    const bool greedy = !(T > 0.f);
    const float* x = xg;
    if ((LOGPROBS || !greedy) && V <= kStageMax) {
        for (int v = threadIdx.x; v < V; v += kThreads) stage[v] = xg[v];
        __syncthreads();
        x = stage;
    }
    int tok;
    if (greedy) {  // the scores as they are, the order and the -FLT_MAX floor of decoder_argmax_kernel
        float mv = -FLT_MAX;
        int mi = -1;
        for (int v = threadIdx.x; v < V; v += kThreads) {
            const float xv = x[v];
            if (xv > mv) {
                mv = xv;
                mi = v;
            }
        }
        tok = block_argmax(mv, mi, sh);
    } else {
        tok = draw_row(x, V, T, K, P, seed, L, sh);
    }
    if constexpr (LOGPROBS) row_logprobs(x, V, tok, out, slot, sh);
    return tok;
}

template <bool LOGPROBS>
__global__ __launch_bounds__(kThreads) void sample_tokens_kernel(
    const float* __restrict__ logits, const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const int64_t* __restrict__ seed, const int* __restrict__ lengths,
    int* __restrict__ tokens, int V, const LogprobOut<LOGPROBS> out) {
    extern __shared__ float stage[];
    __shared__ SampleShared sh;
    const int b = blockIdx.x;
    const int L = lengths[b];
    if (L == 0) {  // empty slot
        if (threadIdx.x == 0) tokens[b] = MLI_EMPTY_ROW_TOKEN_ID;
        if constexpr (LOGPROBS) no_token_logprobs(out, b);
        return;
    }
    const int tok = sample_row<LOGPROBS>(logits + (int64_t)b * V, V, temperature[b], top_k[b], top_p[b], (uint64_t)seed[b],
                                         L, stage, sh, out, b);
    if (threadIdx.x == 0) tokens[b] = tok;
}

// the token pick, then what decoder_finalize_kernel does with it: result, length update, next input embedding
template <bool PAGED, int ELEM, bool LOGPROBS>
__global__ __launch_bounds__(kThreads) void decoder_sample_kernel(
    const float* __restrict__ emb_score, const float* __restrict__ temperature, const int* __restrict__ top_k,
    const float* __restrict__ top_p, const int64_t* __restrict__ seed, int* __restrict__ decoder_result,
    int* __restrict__ lengths, float* __restrict__ inp_embedding, float* const* __restrict__ page_table,
    const float* __restrict__ wpe_table, const float* __restrict__ emb_table, int V, int S, int D,
    int n_decoder_results, int i_decoder, const LogprobOut<LOGPROBS> out) {
    extern __shared__ float stage[];
    __shared__ SampleShared sh;
    const int b = blockIdx.x;
    const int L = lengths[b];
    const int64_t slot = (int64_t)b * n_decoder_results + i_decoder;  // strided like decoder_result
    if (L == 0) {  // empty slot
        if (threadIdx.x == 0) decoder_result[slot] = MLI_EMPTY_ROW_TOKEN_ID;
        if constexpr (LOGPROBS) no_token_logprobs(out, slot);
        return;
    }
    // every thread has read L: sample_row's reductions pass barriers before thread 0 writes the new length
    const int tok = sample_row<LOGPROBS>(emb_score + (int64_t)b * V, V, temperature[b], top_k[b], top_p[b],
                                         (uint64_t)seed[b], L, stage, sh, out, slot);
    const bool done = (L + 1 >= S) || tok == MLI_EOF_TOKEN_ID;
    if (threadIdx.x == 0) {
        decoder_result[slot] = tok;
        lengths[b] = done ? 0 : L + 1;
    }
    if (done || tok < 0) return;  // finished rows get no next embedding
    float* page = nullptr;
    if (PAGED) {
        page = page_table[(int64_t)b * (S / kPage) + L / kPage];
        if (page == nullptr) return;  // no page for the next position (a caller bug): skip rather than fault
    }
    const float4* e = reinterpret_cast<const float4*>(emb_table + (int64_t)tok * D);
    const float4* p = reinterpret_cast<const float4*>(wpe_table + (int64_t)L * D);
    float* dst = !PAGED ? inp_embedding + ((int64_t)b * S + L) * D : page_row_ptr<ELEM>(page, L, D, kSegInp);
    for (int i = threadIdx.x; i < (D >> 2); i += kThreads) store_sum4<ELEM>(dst, i, e[i], p[i]);
}

// The figures of mli_sample_tokens_logprobs for a token the caller GIVES (prompt log-probabilities): row_logprobs on the
// row staged as sample_row stages it, so a target that is the token the head emits reports the same bits.  A target outside
// [0, V) reports -inf for the token and the alternatives all the same.  skipping: a row whose target is no_row belongs to no
// query (mli_paged_prompt_logprobs: a segment the device checks skipped); its logits were never written, and nothing of it is.
__global__ __launch_bounds__(kThreads) void score_tokens_kernel(const float* __restrict__ logits, const int* __restrict__ targets,
                                                                int V, const LogprobOut<true> out, int no_row, bool skipping) {
    extern __shared__ float stage[];
    __shared__ SampleShared sh;
    const int b = blockIdx.x;
    if (skipping && targets[b] == no_row) return;   // workgroup-uniform
    const float* x = logits + (int64_t)b * V;
    if (V <= kStageMax) {
        for (int v = threadIdx.x; v < V; v += kThreads) stage[v] = x[v];
        __syncthreads();
        x = stage;
    }
    const int target = targets[b];
    const bool known = target >= 0 && target < V;
    row_logprobs(x, V, known ? target : 0, out, b, sh);
    if (!known && threadIdx.x == 0) out.token_logprob[b] = -INFINITY;   // (the same thread wrote the stand-in's figure)
}

size_t stage_bytes(int V) { return V <= kStageMax ? (size_t)V * sizeof(float) : 0; }

}  // namespace
}  // namespace mli

extern "C" {

size_t mli_sample_scratch_bytes(int n_batch, int n_vocab) {
    (void)n_batch;
    (void)n_vocab;
    return 0;  // the draw keeps everything in registers and LDS
}

// the refusals of the _logprobs entries, before any device pointer is looked at
static bool logprob_args_ok(const float* token_logprob, const int* top_ids, const float* top_logprobs, int n_top) {
    return n_top >= 0 && n_top <= MLI_MAX_TOP_LOGPROBS && token_logprob != nullptr &&
           (n_top == 0 || (top_ids != nullptr && top_logprobs != nullptr));
}

int mli_sample_tokens(const float* logits, const float* temperature, const int* top_k, const float* top_p,
                      const int64_t* seed, const int* lengths, int* tokens, int n_batch, int n_vocab, void* scratch,
                      size_t scratch_bytes, void* stream) {
    (void)scratch;
    (void)scratch_bytes;
    if (n_batch <= 0 || n_vocab <= 0) return MLI_ERR_BAD_ARG;
    hipLaunchKernelGGL(mli::sample_tokens_kernel<false>, dim3(n_batch), dim3(mli::kThreads), mli::stage_bytes(n_vocab),
                       mli::as_stream(stream), logits, temperature, top_k, top_p, seed, lengths, tokens, n_vocab,
                       mli::LogprobOut<false>{});
    return mli::launch_status();
}

int mli_sample_tokens_logprobs(const float* logits, const float* temperature, const int* top_k, const float* top_p,
                               const int64_t* seed, const int* lengths, int* tokens, float* token_logprob, int* top_ids,
                               float* top_logprobs, int n_batch, int n_vocab, int n_top, void* scratch,
                               size_t scratch_bytes, void* stream) {
    (void)scratch;
    (void)scratch_bytes;
    if (!logprob_args_ok(token_logprob, top_ids, top_logprobs, n_top)) return MLI_ERR_BAD_ARG;
    if (n_batch <= 0 || n_vocab <= 0) return MLI_ERR_BAD_ARG;
    hipLaunchKernelGGL(mli::sample_tokens_kernel<true>, dim3(n_batch), dim3(mli::kThreads), mli::stage_bytes(n_vocab),
                       mli::as_stream(stream), logits, temperature, top_k, top_p, seed, lengths, tokens, n_vocab,
                       mli::LogprobOut<true>{token_logprob, top_ids, top_logprobs, n_top});
    return mli::launch_status();
}

int mli_score_tokens_logprobs(const float* logits, const int* targets, float* token_logprob, int* top_ids,
                              float* top_logprobs, int n, int n_vocab, int n_top, void* stream) {
    if (!logprob_args_ok(token_logprob, top_ids, top_logprobs, n_top)) return MLI_ERR_BAD_ARG;
    if (n < 0 || n_vocab <= 0) return MLI_ERR_BAD_ARG;
    if (n == 0) return 0;
    if (logits == nullptr || targets == nullptr) return MLI_ERR_BAD_ARG;
    hipLaunchKernelGGL(mli::score_tokens_kernel, dim3(n), dim3(mli::kThreads), mli::stage_bytes(n_vocab), mli::as_stream(stream),
                       logits, targets, n_vocab, mli::LogprobOut<true>{token_logprob, top_ids, top_logprobs, n_top}, 0, false);
    return mli::launch_status();
}

size_t mli_decoder_sampled_scratch_bytes(int n_batch, int n_vocab) {
    if (n_batch <= 0 || n_vocab <= 0) return 0;
    return (size_t)n_batch * n_vocab * sizeof(float) + mli_sample_scratch_bytes(n_batch, n_vocab);
}

}  // extern "C"

namespace mli {
// mli_score_tokens_logprobs for mli_paged_prompt_logprobs (compose.hip): rows whose target is no_row are left alone
int launch_score_tokens_skipping(const float* logits, const int* targets, float* token_logprob, int* top_ids,
                                float* top_logprobs, int n, int n_vocab, int n_top, int no_row, void* stream) {
    if (!logprob_args_ok(token_logprob, top_ids, top_logprobs, n_top)) return MLI_ERR_BAD_ARG;
    if (n <= 0 || n_vocab <= 0 || logits == nullptr || targets == nullptr) return MLI_ERR_BAD_ARG;
    hipLaunchKernelGGL(score_tokens_kernel, dim3(n), dim3(kThreads), stage_bytes(n_vocab), as_stream(stream),
                       logits, targets, n_vocab, LogprobOut<true>{token_logprob, top_ids, top_logprobs, n_top}, no_row, true);
    return launch_status();
}
}  // namespace mli

// layout: 0 = contiguous (inp_embedding), 1 = paged fp32, 2 = paged bf16, 3 = paged fp8
template <bool LOGPROBS>
static int decoder_sampled(int layout, const float* batch_result, const float* emb_table, const float* wpe_table,
                           float* inp_embedding, float* const* page_table, int* lengths, int* decoder_result,
                           int n_batch, int n_vocab, int n_sequence, int emb_dim, int n_decoder_results, int i_decoder,
                           const float* temperature, const int* top_k, const float* top_p, const int64_t* seed,
                           void* scratch, size_t scratch_bytes, void* stream, const mli::LogprobOut<LOGPROBS>& out) {
    if (emb_dim % (layout == 3 ? 16 : layout == 2 ? 8 : 4) != 0 || n_batch <= 0 || n_vocab <= 0 || n_decoder_results <= 0 ||
        i_decoder < 0 || i_decoder >= n_decoder_results || (layout != 0 && n_sequence % mli::kPage != 0))
        return MLI_ERR_BAD_ARG;
    if (scratch == nullptr || scratch_bytes < mli_decoder_sampled_scratch_bytes(n_batch, n_vocab)) return MLI_ERR_WORKSPACE;
    hipStream_t st = mli::as_stream(stream);
    float* emb_score = reinterpret_cast<float*>(scratch);
    int rc = mli::launch_gemm_nt(batch_result, emb_table, emb_score, n_batch, n_vocab, emb_dim, st);
    if (rc) return rc;
    const dim3 grid(n_batch), block(mli::kThreads);
    const size_t lds = mli::stage_bytes(n_vocab);
#define MLI_SAMPLE_HEAD(PAGED, ELEM)                                                                                       \
    hipLaunchKernelGGL((mli::decoder_sample_kernel<PAGED, ELEM, LOGPROBS>), grid, block, lds, st, emb_score, temperature,  \
                       top_k, top_p, seed, decoder_result, lengths, inp_embedding, page_table, wpe_table, emb_table,       \
                       n_vocab, n_sequence, emb_dim, n_decoder_results, i_decoder, out)
    if (layout == 0) MLI_SAMPLE_HEAD(false, MLI_ELEM_F32);
    else if (layout == 1) MLI_SAMPLE_HEAD(true, MLI_ELEM_F32);
    else if (layout == 2) MLI_SAMPLE_HEAD(true, MLI_ELEM_BF16);
    else MLI_SAMPLE_HEAD(true, MLI_ELEM_FP8);
#undef MLI_SAMPLE_HEAD
    return mli::launch_status();
}

extern "C" {

int mli_decoder_sampled(const float* batch_result, const float* emb_table, const float* wpe_table, float* inp_embedding,
                        int* lengths, int* decoder_result, int n_batch, int n_vocab, int n_sequence, int emb_dim,
                        const float* temperature, const int* top_k, const float* top_p, const int64_t* seed,
                        void* scratch, size_t scratch_bytes, void* stream) {
    return decoder_sampled<false>(0, batch_result, emb_table, wpe_table, inp_embedding, nullptr, lengths, decoder_result,
                                  n_batch, n_vocab, n_sequence, emb_dim, 1, 0, temperature, top_k, top_p, seed, scratch,
                                  scratch_bytes, stream, {});
}

int mli_paged_decoder_sampled(const float* batch_result, const float* emb_table, const float* wpe_table,
                              void* const* page_table, int* lengths, int* decoder_result, int n_batch, int n_vocab,
                              int n_sequence, int emb_dim, int n_decoder_results, int i_decoder, int elem,
                              const float* temperature, const int* top_k, const float* top_p, const int64_t* seed,
                              void* scratch, size_t scratch_bytes, void* stream) {
    if (elem < MLI_ELEM_F32 || elem > MLI_ELEM_FP8) return MLI_ERR_BAD_ARG;
    return decoder_sampled<false>(1 + elem, batch_result, emb_table, wpe_table, nullptr,
                                  reinterpret_cast<float* const*>(page_table), lengths, decoder_result, n_batch, n_vocab,
                                  n_sequence, emb_dim, n_decoder_results, i_decoder, temperature, top_k, top_p, seed, scratch,
                                  scratch_bytes, stream, {});
}

int mli_decoder_sampled_logprobs(const float* batch_result, const float* emb_table, const float* wpe_table,
                                 float* inp_embedding, int* lengths, int* decoder_result, int n_batch, int n_vocab,
                                 int n_sequence, int emb_dim, int n_decoder_results, int i_decoder,
                                 const float* temperature, const int* top_k, const float* top_p, const int64_t* seed,
                                 float* token_logprob, int* top_ids, float* top_logprobs, int n_top, void* scratch,
                                 size_t scratch_bytes, void* stream) {
    if (!logprob_args_ok(token_logprob, top_ids, top_logprobs, n_top)) return MLI_ERR_BAD_ARG;
    return decoder_sampled<true>(0, batch_result, emb_table, wpe_table, inp_embedding, nullptr, lengths, decoder_result,
                                 n_batch, n_vocab, n_sequence, emb_dim, n_decoder_results, i_decoder, temperature, top_k,
                                 top_p, seed, scratch, scratch_bytes, stream, {token_logprob, top_ids, top_logprobs, n_top});
}

int mli_paged_decoder_sampled_logprobs(const float* batch_result, const float* emb_table, const float* wpe_table,
                                       void* const* page_table, int* lengths, int* decoder_result, int n_batch,
                                       int n_vocab, int n_sequence, int emb_dim, int n_decoder_results, int i_decoder,
                                       int elem, const float* temperature, const int* top_k, const float* top_p,
                                       const int64_t* seed, float* token_logprob, int* top_ids, float* top_logprobs,
                                       int n_top, void* scratch, size_t scratch_bytes, void* stream) {
    if (!logprob_args_ok(token_logprob, top_ids, top_logprobs, n_top)) return MLI_ERR_BAD_ARG;
    if (elem < MLI_ELEM_F32 || elem > MLI_ELEM_FP8) return MLI_ERR_BAD_ARG;
    return decoder_sampled<true>(1 + elem, batch_result, emb_table, wpe_table, nullptr,
                                 reinterpret_cast<float* const*>(page_table), lengths, decoder_result, n_batch, n_vocab,
                                 n_sequence, emb_dim, n_decoder_results, i_decoder, temperature, top_k, top_p, seed, scratch,
                                 scratch_bytes, stream, {token_logprob, top_ids, top_logprobs, n_top});
}

}  // extern "C"
