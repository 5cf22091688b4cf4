// fp32 MFMA GEMM core for every dense product on the decode path:
//   * decode projection   x[B,D] . [Wk|Wq|Wv]   with gather prologue + page/cache scatter epilogue
//       replaces get_latest_kt_q_v                  (src/kernels/self_attention_inference_optimized.cu:100-143)
//                get_latest_k_q_v_paged_attention   (src/kernels/paged_attention.cu:126-180)
//                get_latest_batch_embs + 3 x cublasSgemm + save_to_page_table
//                                                   (src/kernels/paged_attention_cublas.cu:16-99)
//   * prefill fill        X_b[L_b,D] . [Wk|Wv]  for newly inserted rows
//       replaces fill_new_kt_v_cache                (…optimized.cu:27-85)
//                fill_new_k_v_cache_paged_attention (paged_attention.cu:20-87)
//                fill_new_k_v_cache_paged_attention_warp_tiling (paged_attention_cublas.cu:112-223)
//   * decoder logits      attn[B,D] . emb_table[V,D]^T
//       replaces gemm_transpose_kernel (src/kernels/gemm.cu:13-51) / cublasSgemm (src/kernels/decoder.cu:247-249)
//
// v_mfma_f32_32x32x2_f32 is an exact, k-ordered fp32 fma chain, so results are fp32-faithful
// (no TF32-style truncation).  Tile: 64x64x32 per 256-thread workgroup, 2x2 waves of 32x32.
// Per-row source / destination pointers are resolved once per workgroup into LDS (this is where
// the page table is read: one pointer per row, never inside the k loop).
#include "gemm_common.hpp"

namespace mli {

constexpr int BM = 64, BN = 64;   // (rows per workgroup and the k extent of a staged tile are set inside the kernel)
constexpr int LDB = BN + 4;   // [k][n] tile written with b128 stores: rows stay 16-byte aligned
constexpr int LDBT = BN + 1;  // [n][k] source (transposed B): same treatment as A
constexpr int kGemmThreads = 256;

using f32x16 = __attribute__((ext_vector_type(16))) float;

// the tiled kernel, and (EXTENSION) the same kernel with rotary position embeddings in its epilogue
#define MLI_GEMM_ROPE 0
#include "gemm_f32_tile_body.hpp"
#undef MLI_GEMM_ROPE
#define MLI_GEMM_ROPE 1
#include "gemm_f32_tile_body.hpp"
#undef MLI_GEMM_ROPE

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static thread_local int g_fill_compact = 1;  // mli_tune "fill_compact": 0 = one tile grid per new row (the reference's decomposition)
void set_fill_compact(int v) { g_fill_compact = v != 0; }
int fill_compact(int n_new) { return g_fill_compact && n_new <= kMaxCompactRows ? 1 : 0; }
// mli_tune "latest_compact": 0 = the decode projection multiplies empty rows as zeros, 1 (default) = it multiplies a
// device-built list of the non-empty rows where that can pay, 2 = wherever possible (tests).  Every workgroup rebuilds the
// list (a prefix sum over the batch rows): ~1.8 us of prologue -- config 4's projection (emb_dim 512) takes 9.4 us without
// it and 11.2 with it, and could save 3-4 us at best from a batch that is 40 % empty slots; at emb_dim 2048 (222 us) the same
// batch saves 90 us.  So: only for reductions of 1024 and more.
static thread_local int g_latest_compact = 1;
void set_latest_compact(int v) { g_latest_compact = v < 0 ? 0 : (v > 2 ? 2 : v); }
int latest_compact(int n_batch, int k_dim) {
    if (g_latest_compact == 0 || n_batch > kMaxCompactRows) return 0;
    return g_latest_compact == 2 || k_dim >= 1024 ? 1 : 0;
}

// mli_tune "prefill_fused": which form mli_[paged_]prefill runs: 1 (default) = the encoder as the fill GEMM's prologue up to
// emb_dim 512 and encoder + fill as two launches beyond, 0 = always the two launches, 2 = always the prologue form
// (mli_prefill: an input_dim that is no multiple of 4 has the prologue form only, under every setting)
static thread_local int g_prefill_fused = 1;
void set_prefill_fused(int v) { g_prefill_fused = v < 0 ? 0 : (v > 2 ? 2 : v); }
bool prefill_fuses(int emb_dim) { return g_prefill_fused == 2 || (g_prefill_fused == 1 && emb_dim <= 512); }

static thread_local int g_gemm_split = 1;  // mli_tune "gemm_split": 0 = never the loader / MFMA wave split of the 64-row-tile kernel
void set_gemm_split(int v) { g_gemm_split = v != 0; }
static thread_local int g_gemm_tall_tiles = 1;  // mli_tune "gemm_tall_tiles": 0 = always 64-row tiles, 2 = 128-row tiles whenever allowed (tests)
void set_gemm_tall_tiles(int v) { g_gemm_tall_tiles = v < 0 ? 0 : (v > 2 ? 2 : v); }
bool gemm_use_tall_tiles(int64_t tall_workgroups) { return g_gemm_tall_tiles == 2 || (g_gemm_tall_tiles == 1 && tall_workgroups >= 512); }

// proj_gemm_panel.hip: the latency-shaped kernel for small decode-step products
bool gemm_panel_wanted(int M, int N_total, int K, bool vec4);
int gemm_panel_tiles_n(int N);
template <int MODE, bool BT>
int launch_gemm_panel(const GemmArgs& g, int rows, hipStream_t st);

// the launch counters beside the kernel's family: the row list a projection or a fill of the tiled kernels runs over
template <int MODE>
static void count_gemm_form(const GemmArgs& g) {
    constexpr bool kFill = MODE == kNaiveFill || MODE == kPagedFill || MODE == kPagedFillLive;
    if (kFill) count_launch(g.compact ? kLfFillFlat : kLfFillPerRow);
    else if ((MODE == kPagedLatest || MODE == kNaiveLatest) && g.compact) count_launch(kLfLatestCompact);
}

// EXTENSION: the rotary table of a *_rope entry point (null: none) and hd / 2.  With a table the launchers below take the tiled
// kernels' ROPE instantiations -- also at the shapes of the panel kernel, which has no such switch -- and count
// "gemm_f32_rope" beside the family of the form that ran.
struct RopeArg {
    const float2* table = nullptr;
    int half = 0;
};

// the tiled kernels' forms with the rotation, chosen as launch_gemm chooses below
template <int MODE>
static int launch_gemm_rope(const GemmArgs& g, int rows, int z, bool vec4, RopeArg rope, hipStream_t st) {
    const int tiles_x = ceil_div_i(g.N, BN) * g.n_out;
    count_gemm_form<MODE>(g);
    count_launch(kLfGemmF32Rope);
    if constexpr (MODE == kPagedLatest) {  // as in launch_gemm: the fills keep 64-row tiles
        if (vec4 && gemm_use_tall_tiles((int64_t)tiles_x * ceil_div_i(rows, 128) * z)) {
            count_launch(kLfGemmF32Rows128);
            hipLaunchKernelGGL((gemm_f32_mfma_rope_kernel<MODE, false, true, false, 2>), dim3(tiles_x, ceil_div_i(rows, 128), z),
                               dim3(kGemmThreads), 0, st, g, rope.table, rope.half);
            return launch_status();
        }
    }
    dim3 grid(tiles_x, ceil_div_i(rows, BM), z);
    if (g.compact && MODE != kPagedLatest) grid = dim3(tiles_x, ceil_div_i(rows * z, BM), 1);
    if (vec4 && g_gemm_split && g.K >= 256) {
        count_launch(kLfGemmF32Rows64Split);
        hipLaunchKernelGGL((gemm_f32_mfma_rope_kernel<MODE, false, true, false, 1, true>), grid, dim3(2 * kGemmThreads), 0, st, g,
                           rope.table, rope.half);
        return launch_status();
    }
    count_launch(kLfGemmF32Rows64);
    if (vec4) hipLaunchKernelGGL((gemm_f32_mfma_rope_kernel<MODE, false, true>), grid, dim3(kGemmThreads), 0, st, g, rope.table, rope.half);
    else hipLaunchKernelGGL((gemm_f32_mfma_rope_kernel<MODE, false, false>), grid, dim3(kGemmThreads), 0, st, g, rope.table, rope.half);
    return launch_status();
}

// rows = live extent of the M dimension (per z-slice)
template <int MODE, bool BT>
static int launch_gemm(const GemmArgs& g, int rows, int z, bool vec4, hipStream_t st, RopeArg rope = {}) {
    if (g.N <= 0 || g.K <= 0 || rows <= 0 || z <= 0) return MLI_ERR_BAD_ARG;
    if constexpr (!BT && (MODE == kPagedLatest || MODE == kPagedFill || MODE == kPagedFillLive)) {
        if (rope.table != nullptr) return launch_gemm_rope<MODE>(g, rows, z, vec4, rope, st);
    }
    constexpr bool kPanelMode = ((MODE == kPagedLatest || MODE == kNaiveLatest) && !BT) || (MODE == kPlain && BT);
    if constexpr (kPanelMode) {
        if (z == 1 && gemm_panel_wanted(rows, g.N * g.n_out, g.K, vec4)) return launch_gemm_panel<MODE, BT>(g, rows, st);
    }
    const int tiles_x = ceil_div_i(g.N, BN) * g.n_out;
    count_gemm_form<MODE>(g);
    // 128-row tiles when they still fill the chip (>= 2 workgroups per CU) -- decode projection / logits of a large
    // batch; the prefill fill keeps 64-row tiles (a new row's prompt rarely fills 128 rows)
    constexpr bool kTallOk = MODE == kPagedLatest || MODE == kNaiveLatest || MODE == kPlain;
    if constexpr (kTallOk) {   // (if constexpr: the fills instantiate no 128-row kernel that nothing can launch)
        if (vec4 && gemm_use_tall_tiles((int64_t)tiles_x * ceil_div_i(rows, 128) * z)) {
            dim3 grid(tiles_x, ceil_div_i(rows, 128), z);
            count_launch(kLfGemmF32Rows128);
            hipLaunchKernelGGL((gemm_f32_mfma_kernel<MODE, BT, true, false, 2>), grid, dim3(kGemmThreads), 0, st, g);
            return launch_status();
        }
    }
    dim3 grid(tiles_x, ceil_div_i(rows, BM), z);
    if (g.compact && (MODE == kNaiveFill || MODE == kPagedFill || MODE == kPagedFillLive))
        grid = dim3(tiles_x, ceil_div_i(rows * z, BM), 1);  // flat (new row, token) list: upper bound
    // a reduction long enough to pipeline: loader waves + MFMA waves (512 threads).  Measured at D = 2048: logits of 1024
    // rows 61 -> 52 us, prefill of 128 / 256 / 512 / 4096 prompt tokens 60 -> 49 / 63 -> 52 / 96 -> 86 / 593 -> 588 us,
    // config 4 logits (K = 512) 21.4 -> 19.5 us: never slower
    if (vec4 && g_gemm_split && g.K >= 256) {
        count_launch(kLfGemmF32Rows64Split);
        hipLaunchKernelGGL((gemm_f32_mfma_kernel<MODE, BT, true, false, 1, true>), grid, dim3(2 * kGemmThreads), 0, st, g);
        return launch_status();
    }
    count_launch(kLfGemmF32Rows64);
    if (vec4) hipLaunchKernelGGL((gemm_f32_mfma_kernel<MODE, BT, true>), grid, dim3(kGemmThreads), 0, st, g);
    else hipLaunchKernelGGL((gemm_f32_mfma_kernel<MODE, BT, false>), grid, dim3(kGemmThreads), 0, st, g);
    return launch_status();
}

int launch_latest_naive(const float* inp, const int* lengths, const float* wk, const float* wq, const float* wv,
                        float* kt, float* v, float* q, int B, int S, int Din, int Dout, hipStream_t st) {
    if (B <= 0) return MLI_ERR_BAD_ARG;
    GemmArgs g{};
    g.w[0] = wk; g.w[1] = wq; g.w[2] = wv; g.n_out = 3;
    g.out_id[0] = 0; g.out_id[1] = 1; g.out_id[2] = 2;
    g.M = B; g.N = Dout; g.K = Din;
    g.inp_embedding = inp; g.kt_cache = kt; g.v_cache = v; g.q_output = q; g.lengths = lengths;
    g.B = B; g.S = S;
    g.compact = latest_compact(B, Din);
    const bool vec4 = Din % 4 == 0 && Dout % 4 == 0 && aligned16(inp) && aligned16(wk) && aligned16(wq) && aligned16(wv);
    return launch_gemm<kNaiveLatest, false>(g, B, 1, vec4, st);
}

// emb_table != nullptr: the encoder runs as the GEMM's prologue (inp_embedding rows are written, not read)
int launch_fill_naive_embed(const float* emb_table, const float* wpe, const int* tokens, float* inp, const int* new_idx,
                            const int* lengths, const float* wk, const float* wv, float* kt, float* v, int B, int S,
                            int Din, int Dout, int n_new, hipStream_t st) {
    if (n_new == 0) return 0;  // reference …optimized.cu:308-310
    if (n_new < 0 || B <= 0) return MLI_ERR_BAD_ARG;
    GemmArgs g{};
    g.emb_table = emb_table; g.wpe = wpe; g.inp = tokens;
    g.w[0] = wk; g.w[1] = wv; g.n_out = 2;
    g.out_id[0] = 0; g.out_id[1] = 2;
    g.M = S; g.N = Dout; g.K = Din;
    g.inp_embedding = inp; g.kt_cache = kt; g.v_cache = v; g.lengths = lengths; g.new_batch_idx = new_idx;
    g.B = B; g.S = S;
    g.n_new = n_new; g.compact = fill_compact(n_new);
    const bool vec4 = Din % 4 == 0 && Dout % 4 == 0 && aligned16(inp) && aligned16(wk) && aligned16(wv) &&
                      (emb_table == nullptr || (aligned16(emb_table) && aligned16(wpe)));
    return launch_gemm<kNaiveFill, false>(g, S, n_new, vec4, st);
}

int launch_fill_naive(const float* inp, const int* new_idx, const int* lengths, const float* wk, const float* wv,
                      float* kt, float* v, int B, int S, int Din, int Dout, int n_new, hipStream_t st) {
    return launch_fill_naive_embed(nullptr, nullptr, nullptr, const_cast<float*>(inp), new_idx, lengths, wk, wv, kt, v, B,
                                   S, Din, Dout, n_new, st);
}

static int latest_paged(float* const* page_table, const int* lengths, const float* wk, const float* wq, const float* wv, float* q,
                        int B, int S, int D, RopeArg rope, hipStream_t st) {
    if (B <= 0 || S % kPage != 0 || D % 4 != 0) return MLI_ERR_BAD_ARG;
    GemmArgs g{};
    g.w[0] = wk; g.w[1] = wq; g.w[2] = wv; g.n_out = 3;
    g.out_id[0] = 0; g.out_id[1] = 1; g.out_id[2] = 2;
    g.M = B; g.N = D; g.K = D;
    g.page_table = page_table; g.q_output = q; g.lengths = lengths;
    g.B = B; g.S = S;
    g.compact = latest_compact(B, D);
    const bool vec4 = aligned16(wk) && aligned16(wq) && aligned16(wv);
    return launch_gemm<kPagedLatest, false>(g, B, 1, vec4, st, rope);
}

int launch_latest_paged(float* const* page_table, const int* lengths, const float* wk, const float* wq,
                        const float* wv, float* q, int B, int S, int D, hipStream_t st) {
    return latest_paged(page_table, lengths, wk, wq, wv, q, B, S, D, RopeArg{}, st);
}

// WIN: the windowed prefill's fill (1 <= window, 0 <= n_sink, n_sink + window < S: the entry point hands everything else on)
template <bool WIN>
static int fill_paged_embed(const float* emb_table, const float* wpe, const int* tokens, float* const* page_table,
                            const int* new_idx, const int* lengths, const float* wk, const float* wv, int B, int S, int D,
                            int n_new, int window, int n_sink, hipStream_t st, RopeArg rope = {}) {
    if (n_new == 0) return 0;  // reference paged_attention.cu:100-102
    if (n_new < 0 || B <= 0 || S % kPage != 0 || D % 4 != 0) return MLI_ERR_BAD_ARG;
    GemmArgs g{};
    g.emb_table = emb_table; g.wpe = wpe; g.inp = tokens;
    g.w[0] = wk; g.w[1] = wv; g.n_out = 2;
    g.out_id[0] = 0; g.out_id[1] = 2;
    g.M = S; g.N = D; g.K = D;
    g.page_table = page_table; g.lengths = lengths; g.new_batch_idx = new_idx;
    g.B = B; g.S = S;
    g.n_new = n_new; g.compact = fill_compact(n_new);
    const bool vec4 = aligned16(wk) && aligned16(wv) && (emb_table == nullptr || (aligned16(emb_table) && aligned16(wpe)));
    if (!WIN) return launch_gemm<kPagedFill, false>(g, S, n_new, vec4, st, rope);
    g.fill_window = window; g.fill_sink = n_sink;
    // the flat list is at most live_tokens_bound pairs per row; the per-row grid keeps the row's extent
    return launch_gemm<kPagedFillLive, false>(g, g.compact ? live_tokens_bound(S, window, n_sink) : S, n_new, vec4, st, rope);
}

int launch_fill_paged_embed(const float* emb_table, const float* wpe, const int* tokens, float* const* page_table,
                            const int* new_idx, const int* lengths, const float* wk, const float* wv, int B, int S, int D,
                            int n_new, hipStream_t st) {
    return fill_paged_embed<false>(emb_table, wpe, tokens, page_table, new_idx, lengths, wk, wv, B, S, D, n_new, 0, 0, st);
}

int launch_fill_paged_window_embed(const float* emb_table, const float* wpe, const int* tokens, float* const* page_table,
                                   const int* new_idx, const int* lengths, const float* wk, const float* wv, int B, int S,
                                   int D, int n_new, int window, int n_sink, hipStream_t st) {
    return fill_paged_embed<true>(emb_table, wpe, tokens, page_table, new_idx, lengths, wk, wv, B, S, D, n_new, window, n_sink, st);
}

int launch_fill_paged(float* const* page_table, const int* new_idx, const int* lengths, const float* wk,
                      const float* wv, int B, int S, int D, int n_new, hipStream_t st) {
    return launch_fill_paged_embed(nullptr, nullptr, nullptr, page_table, new_idx, lengths, wk, wv, B, S, D, n_new, st);
}

// bf16 tile engine: 1 = native v_mfma_f32_32x32x16_bf16 (proj_gemm_bf16.hip, default), 0 = operands widened to
// fp32 in LDS + fp32 MFMA (bit-identical to a sequential fp32 sum; kept for parity checks).  mli_tune knob.
static thread_local int g_bf16_native_mfma = 1;
void set_bf16_native_mfma(int v) { g_bf16_native_mfma = v != 0; }
int launch_latest_paged_bf16_native(uint16_t* const*, const int*, const uint16_t*, const uint16_t*, const uint16_t*,
                                    float*, int, int, int, hipStream_t);
int launch_fill_paged_bf16_native(uint16_t* const*, const int*, const int*, const uint16_t*, const uint16_t*, int, int,
                                  int, int, hipStream_t);
// proj_gemm_bf16.hip, EXTENSION: the native kernels' ROPE forms (table: [S][half] (cos, sin))
int launch_latest_paged_16bit_rope(void* const*, const int*, const uint16_t*, const uint16_t*, const uint16_t*, float*, int, int,
                                   int, const float2*, int, bool, hipStream_t);
int launch_fill_paged_16bit_rope(const float*, const float*, const int*, void* const*, const int*, const int*, const uint16_t*,
                                 const uint16_t*, int, int, int, int, int, int, const float2*, int, bool, hipStream_t);

static int latest_paged_bf16(uint16_t* const* page_table, const int* lengths, const uint16_t* wk, const uint16_t* wq,
                             const uint16_t* wv, float* q, int B, int S, int D, RopeArg rope, hipStream_t st) {
    if (B <= 0 || S % kPage != 0 || D % 8 != 0) return MLI_ERR_BAD_ARG;
    if (g_bf16_native_mfma) {
        if (rope.table != nullptr)
            return launch_latest_paged_16bit_rope(reinterpret_cast<void* const*>(page_table), lengths, wk, wq, wv, q, B, S, D,
                                                  rope.table, rope.half, false, st);
        return launch_latest_paged_bf16_native(page_table, lengths, wk, wq, wv, q, B, S, D, st);
    }
    GemmArgs g{};
    g.w[0] = reinterpret_cast<const float*>(wk); g.w[1] = reinterpret_cast<const float*>(wq);
    g.w[2] = reinterpret_cast<const float*>(wv); g.n_out = 3;
    g.out_id[0] = 0; g.out_id[1] = 1; g.out_id[2] = 2;
    g.M = B; g.N = D; g.K = D;
    g.page_table = reinterpret_cast<float* const*>(page_table); g.q_output = q; g.lengths = lengths;
    g.B = B; g.S = S;
    g.compact = latest_compact(B, D);
    dim3 grid(ceil_div_i(D, BN) * 3, ceil_div_i(B, BM), 1);
    count_launch(kLfGemmBf16Widened);
    count_gemm_form<kPagedLatest>(g);
    if (rope.table != nullptr) {
        count_launch(kLfGemmF32Rope);
        hipLaunchKernelGGL((gemm_f32_mfma_rope_kernel<kPagedLatest, false, true, true>), grid, dim3(kGemmThreads), 0, st, g, rope.table,
                           rope.half);
        return launch_status();
    }
    hipLaunchKernelGGL((gemm_f32_mfma_kernel<kPagedLatest, false, true, true>), grid, dim3(kGemmThreads), 0, st, g);
    return launch_status();
}

int launch_latest_paged_bf16(uint16_t* const* page_table, const int* lengths, const uint16_t* wk,
                             const uint16_t* wq, const uint16_t* wv, float* q, int B, int S, int D, hipStream_t st) {
    return latest_paged_bf16(page_table, lengths, wk, wq, wv, q, B, S, D, RopeArg{}, st);
}

int launch_fill_paged_bf16_window_embed(const float*, const float*, const int*, uint16_t* const*, const int*, const int*,
                                        const uint16_t*, const uint16_t*, int, int, int, int, int, int, hipStream_t);

template <bool WIN>
static int fill_paged_bf16(uint16_t* const* page_table, const int* new_idx, const int* lengths, const uint16_t* wk,
                           const uint16_t* wv, int B, int S, int D, int n_new, int window, int n_sink, hipStream_t st,
                           RopeArg rope = {}) {
    if (n_new == 0) return 0;
    if (n_new < 0 || B <= 0 || S % kPage != 0 || D % 8 != 0) return MLI_ERR_BAD_ARG;
    if (g_bf16_native_mfma && rope.table != nullptr)
        return launch_fill_paged_16bit_rope(nullptr, nullptr, nullptr, reinterpret_cast<void* const*>(page_table), new_idx, lengths,
                                            wk, wv, B, S, D, n_new, WIN ? window : 0, n_sink, rope.table, rope.half, false, st);
    if (g_bf16_native_mfma)
        return WIN ? launch_fill_paged_bf16_window_embed(nullptr, nullptr, nullptr, page_table, new_idx, lengths, wk, wv, B, S,
                                                         D, n_new, window, n_sink, st)
                   : launch_fill_paged_bf16_native(page_table, new_idx, lengths, wk, wv, B, S, D, n_new, st);
    GemmArgs g{};
    g.w[0] = reinterpret_cast<const float*>(wk); g.w[1] = reinterpret_cast<const float*>(wv); g.n_out = 2;
    g.out_id[0] = 0; g.out_id[1] = 2;
    g.M = S; g.N = D; g.K = D;
    g.page_table = reinterpret_cast<float* const*>(page_table); g.lengths = lengths; g.new_batch_idx = new_idx;
    g.B = B; g.S = S;
    g.n_new = n_new; g.compact = fill_compact(n_new);
    dim3 grid(ceil_div_i(D, BN) * 2, ceil_div_i(S, BM), n_new);
    count_launch(kLfGemmBf16Widened);
    count_gemm_form<kPagedFill>(g);
    if (rope.table != nullptr) count_launch(kLfGemmF32Rope);
    if (!WIN) {
        if (g.compact) grid = dim3(ceil_div_i(D, BN) * 2, ceil_div_i(S * n_new, BM), 1);
        if (rope.table != nullptr)
            hipLaunchKernelGGL((gemm_f32_mfma_rope_kernel<kPagedFill, false, true, true>), grid, dim3(kGemmThreads), 0, st, g, rope.table,
                               rope.half);
        else
            hipLaunchKernelGGL((gemm_f32_mfma_kernel<kPagedFill, false, true, true>), grid, dim3(kGemmThreads), 0, st, g);
        return launch_status();
    }
    g.fill_window = window; g.fill_sink = n_sink;
    if (g.compact) grid = dim3(ceil_div_i(D, BN) * 2, ceil_div_i(live_tokens_bound(S, window, n_sink) * n_new, BM), 1);
    if (rope.table != nullptr)
        hipLaunchKernelGGL((gemm_f32_mfma_rope_kernel<kPagedFillLive, false, true, true>), grid, dim3(kGemmThreads), 0, st, g, rope.table,
                           rope.half);
    else
        hipLaunchKernelGGL((gemm_f32_mfma_kernel<kPagedFillLive, false, true, true>), grid, dim3(kGemmThreads), 0, st, g);
    return launch_status();
}

int launch_fill_paged_bf16(uint16_t* const* page_table, const int* new_idx, const int* lengths, const uint16_t* wk,
                           const uint16_t* wv, int B, int S, int D, int n_new, hipStream_t st) {
    return fill_paged_bf16<false>(page_table, new_idx, lengths, wk, wv, B, S, D, n_new, 0, 0, st);
}

int launch_fill_paged_bf16_window(uint16_t* const* page_table, const int* new_idx, const int* lengths, const uint16_t* wk,
                                  const uint16_t* wv, int B, int S, int D, int n_new, int window, int n_sink, hipStream_t st) {
    return fill_paged_bf16<true>(page_table, new_idx, lengths, wk, wv, B, S, D, n_new, window, n_sink, st);
}

// ---- EXTENSION: rotary position embeddings (the *_rope entry points, include/mli_kernels.h) ---------------------------------
// hd / 2 for a table that can be used, -1 for what every *_rope call refuses before it launches anything
int rope_half(int D, int n_heads, const float* table) {
    if (table == nullptr || n_heads < 1 || D < 1 || D % n_heads != 0 || (D / n_heads) % 2 != 0) return -1;
    return D / n_heads / 2;
}

int launch_latest_paged_rope(int elem, void* const* page_table, const int* lengths, const void* wk, const void* wq,
                             const void* wv, float* q, int B, int S, int D, int n_heads, const float* table, hipStream_t st) {
    const int half = rope_half(D, n_heads, table);
    if (half < 0) return MLI_ERR_BAD_ARG;
    const RopeArg rope{reinterpret_cast<const float2*>(table), half};
    const uint16_t *k16 = static_cast<const uint16_t*>(wk), *q16 = static_cast<const uint16_t*>(wq), *v16 = static_cast<const uint16_t*>(wv);
    if (elem == MLI_ELEM_FP8) return launch_latest_paged_16bit_rope(page_table, lengths, k16, q16, v16, q, B, S, D, rope.table, half, true, st);
    if (elem == MLI_ELEM_BF16)
        return latest_paged_bf16(reinterpret_cast<uint16_t* const*>(page_table), lengths, k16, q16, v16, q, B, S, D, rope, st);
    if (elem == MLI_ELEM_F32)
        return latest_paged(reinterpret_cast<float* const*>(page_table), lengths, static_cast<const float*>(wk),
                            static_cast<const float*>(wq), static_cast<const float*>(wv), q, B, S, D, rope, st);
    return MLI_ERR_BAD_ARG;
}

// emb_table null: the x rows are read from segment 0; else the encoder is the fill's prologue.  win: the windowed prefill's live
// fill (the caller has held 1 <= window, 0 <= n_sink, n_sink + window < S), else every token of a new row.
int launch_fill_paged_rope(int elem, const float* emb_table, const float* wpe, const int* tokens, void* const* page_table,
                           const int* new_idx, const int* lengths, const void* wk, const void* wv, int B, int S, int D, int n_new,
                           bool win, int window, int n_sink, int n_heads, const float* table, hipStream_t st) {
    const int half = rope_half(D, n_heads, table);
    if (half < 0 || (win && (window < 1 || n_sink < 0 || (int64_t)n_sink + window >= S))) return MLI_ERR_BAD_ARG;
    const RopeArg rope{reinterpret_cast<const float2*>(table), half};
    const uint16_t *k16 = static_cast<const uint16_t*>(wk), *v16 = static_cast<const uint16_t*>(wv);
    if (elem == MLI_ELEM_FP8 || (elem == MLI_ELEM_BF16 && emb_table != nullptr))
        return launch_fill_paged_16bit_rope(emb_table, wpe, tokens, page_table, new_idx, lengths, k16, v16, B, S, D, n_new,
                                            win ? window : 0, n_sink, rope.table, half, elem == MLI_ELEM_FP8, st);
    if (elem == MLI_ELEM_BF16) {
        uint16_t* const* pt = reinterpret_cast<uint16_t* const*>(page_table);
        return win ? fill_paged_bf16<true>(pt, new_idx, lengths, k16, v16, B, S, D, n_new, window, n_sink, st, rope)
                   : fill_paged_bf16<false>(pt, new_idx, lengths, k16, v16, B, S, D, n_new, 0, 0, st, rope);
    }
    if (elem == MLI_ELEM_F32) {
        float* const* pt = reinterpret_cast<float* const*>(page_table);
        const float *k = static_cast<const float*>(wk), *v = static_cast<const float*>(wv);
        return win ? fill_paged_embed<true>(emb_table, wpe, tokens, pt, new_idx, lengths, k, v, B, S, D, n_new, window, n_sink, st, rope)
                   : fill_paged_embed<false>(emb_table, wpe, tokens, pt, new_idx, lengths, k, v, B, S, D, n_new, 0, 0, st, rope);
    }
    return MLI_ERR_BAD_ARG;
}

// C[M, N] = A[M, K] . Bt[N, K]^T
int launch_gemm_nt(const float* A, const float* Bt, float* C, int M, int N, int K, hipStream_t st) {
    if (M <= 0) return MLI_ERR_BAD_ARG;
    GemmArgs g{};
    g.w[0] = Bt; g.n_out = 1; g.out_id[0] = 1;
    g.M = M; g.N = N; g.K = K;
    g.a_plain = A; g.c_plain = C; g.lda = K; g.ldc = N;
    const bool vec4 = K % 4 == 0 && aligned16(A) && aligned16(Bt);
    return launch_gemm<kPlain, true>(g, M, 1, vec4, st);
}

// Q for prompt positions (attention_prompt.hpp): q[i] = x(row, pos) . Wq for the positions of a list of segments, i =
// seg_offset + j for position seg_first + j of row seg_row.  A gather of the x rows (segment 0 of the pages, where the prefill
// has just written them) into `gathered` ([n_q, D] page elements), then the plain product of this file's template over it: fp32 x
// and Wq, or (BF16) bf16 x and Wq widened to fp32 while they are staged -- the exact k-ordered fp32 MFMA chain either way.
// A position outside its row's pages or the q array gathers nothing; its q row is then whatever `gathered` held -- and so is
// every q row that belongs to no position at all (a hole between segments, a tail, a skipped segment): the product covers all
// n_q rows.  That is this entry point's contract (include/mli_kernels.h); the scan reads the q rows of its queries only.
template <int EB>   // bytes per page element
__global__ __launch_bounds__(256) void prompt_gather_x_kernel(const void* const* __restrict__ page_table,
                                                              const int* __restrict__ seg_row, const int* __restrict__ seg_first,
                                                              const int* __restrict__ seg_count, const int* __restrict__ seg_offset,
                                                              void* __restrict__ gathered, int n_q, int B, int S, int D) {
    const int seg = blockIdx.y, j = blockIdx.x;
    const int cnt = seg_count[seg];
    if (j >= cnt) return;
    const int b = seg_row[seg], first = seg_first[seg], off = seg_offset[seg];
    if (b < 0 || b >= B || first < 0 || (int64_t)first + cnt > S || off < 0 || (int64_t)off + cnt > n_q) return;
    const int s = first + j;
    const char* page = static_cast<const char*>(page_table[(int64_t)b * (S / kPage) + s / kPage]);
    if (page == nullptr) return;
    const uint2* src = reinterpret_cast<const uint2*>(page + page_row_offset(s, D, kSegInp) * EB);   // D * EB % 8 == 0
    uint2* dst = reinterpret_cast<uint2*>(static_cast<char*>(gathered) + ((int64_t)off + j) * D * EB);
    for (int i = threadIdx.x; i < D * EB / 8; i += 256) dst[i] = src[i];
}

int launch_prompt_project_q(int elem, const void* const* page_table, const int* seg_row, const int* seg_first,
                            const int* seg_count, const int* seg_offset, const void* wq, void* gathered, float* q, int n_seg,
                            int max_count, int n_q, int B, int S, int D, hipStream_t st) {
    if ((elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) || n_seg < 0 || B <= 0 || S <= 0 || S % kPage != 0 || D <= 0 ||
        D % (elem == MLI_ELEM_BF16 ? 8 : 4) != 0)
        return MLI_ERR_BAD_ARG;
    if (n_seg == 0) return 0;
    if (max_count < 1 || max_count > S || n_q < 1 || n_seg > 65535) return MLI_ERR_BAD_ARG;
    if (page_table == nullptr || seg_row == nullptr || seg_first == nullptr || seg_count == nullptr || seg_offset == nullptr ||
        wq == nullptr || gathered == nullptr || q == nullptr || !aligned16(wq) || !aligned16(gathered))
        return MLI_ERR_BAD_ARG;
    const bool bf16 = elem == MLI_ELEM_BF16;
    if (bf16)
        hipLaunchKernelGGL(prompt_gather_x_kernel<2>, dim3(max_count, n_seg), dim3(256), 0, st, page_table, seg_row, seg_first,
                           seg_count, seg_offset, gathered, n_q, B, S, D);
    else
        hipLaunchKernelGGL(prompt_gather_x_kernel<4>, dim3(max_count, n_seg), dim3(256), 0, st, page_table, seg_row, seg_first,
                           seg_count, seg_offset, gathered, n_q, B, S, D);
    int rc = launch_status();
    if (rc) return rc;
    GemmArgs g{};
    g.w[0] = static_cast<const float*>(wq); g.n_out = 1; g.out_id[0] = 1;
    g.M = n_q; g.N = D; g.K = D;
    g.a_plain = static_cast<const float*>(gathered); g.c_plain = q;
    g.lda = bf16 ? D / 2 : D;   // in floats: a bf16 row is D / 2 of them
    g.ldc = D;
    const dim3 grid(ceil_div_i(D, BN), ceil_div_i(n_q, BM), 1);
    if (bf16) {
        count_launch(kLfGemmBf16Widened);
        hipLaunchKernelGGL((gemm_f32_mfma_kernel<kPlain, false, true, true>), grid, dim3(kGemmThreads), 0, st, g);
    } else {
        count_launch(kLfGemmF32Rows64);
        hipLaunchKernelGGL((gemm_f32_mfma_kernel<kPlain, false, true>), grid, dim3(kGemmThreads), 0, st, g);
    }
    return launch_status();
}

// The same product with the argmax epilogue: nothing of C[M, N] is stored, row_best[m][t] = (max, lowest index of the
// max) over the columns of tile t.  Tiles per row: gemm_nt_argmax_tiles(N).
// (the panel kernel's tiles are 32 columns wide, the tiled kernel's 64: n_tiles tells the caller which ran)
int gemm_nt_argmax_max_tiles(int N) { return ceil_div_i(N, 32); }
int launch_gemm_nt_argmax(const float* A, const float* Bt, RowBest* row_best, int M, int N, int K, int* n_tiles,
                          hipStream_t st) {
    if (M <= 0 || row_best == nullptr) return MLI_ERR_BAD_ARG;
    {
        const bool vec4 = K % 4 == 0 && aligned16(A) && aligned16(Bt);
        *n_tiles = gemm_panel_wanted(M, N, K, vec4) ? gemm_panel_tiles_n(N) : ceil_div_i(N, BN);
    }
    GemmArgs g{};
    g.w[0] = Bt; g.n_out = 1; g.out_id[0] = 1;
    g.M = M; g.N = N; g.K = K;
    g.a_plain = A; g.c_plain = nullptr; g.lda = K; g.ldc = N;
    g.row_best = row_best;
    const bool vec4 = K % 4 == 0 && aligned16(A) && aligned16(Bt);
    return launch_gemm<kPlain, true>(g, M, 1, vec4, st);
}

}  // namespace mli

extern "C" {

int mli_fill_new_kt_v_cache(const float* inp_embedding, const int* new_batch_idx, const int* lengths,
                            const float* wk, const float* wv, float* kt_cache, float* v_cache, int n_batch,
                            int n_sequence, int input_dim, int output_dim, int n_new_items, void* stream) {
    return mli::launch_fill_naive(inp_embedding, new_batch_idx, lengths, wk, wv, kt_cache, v_cache, n_batch,
                                  n_sequence, input_dim, output_dim, n_new_items, mli::as_stream(stream));
}

int mli_get_latest_kt_q_v(const float* inp_embedding, const int* lengths, const float* wk, const float* wq,
                          const float* wv, float* kt_cache, float* v_cache, float* q_output, int n_batch,
                          int n_sequence, int input_dim, int output_dim, void* stream) {
    return mli::launch_latest_naive(inp_embedding, lengths, wk, wq, wv, kt_cache, v_cache, q_output, n_batch,
                                    n_sequence, input_dim, output_dim, mli::as_stream(stream));
}

int mli_fill_new_k_v_cache_paged(float* const* page_table, const int* new_batch_idx, const int* lengths,
                                 const float* wk, const float* wv, int n_batch, int n_sequence, int emb_dim,
                                 int n_new_items, void* stream) {
    return mli::launch_fill_paged(page_table, new_batch_idx, lengths, wk, wv, n_batch, n_sequence, emb_dim,
                                  n_new_items, mli::as_stream(stream));
}

int mli_get_latest_k_q_v_paged(float* const* page_table, const int* lengths, const float* wk, const float* wq,
                               const float* wv, float* q_output, int n_batch, int n_sequence, int emb_dim,
                               void* stream) {
    return mli::launch_latest_paged(page_table, lengths, wk, wq, wv, q_output, n_batch, n_sequence, emb_dim,
                                    mli::as_stream(stream));
}

int mli_fill_new_k_v_cache_paged_bf16(mli_bf16* const* page_table, const int* new_batch_idx, const int* lengths,
                                      const mli_bf16* wk, const mli_bf16* wv, int n_batch, int n_sequence,
                                      int emb_dim, int n_new_items, void* stream) {
    return mli::launch_fill_paged_bf16(page_table, new_batch_idx, lengths, wk, wv, n_batch, n_sequence, emb_dim,
                                       n_new_items, mli::as_stream(stream));
}

int mli_get_latest_k_q_v_paged_bf16(mli_bf16* const* page_table, const int* lengths, const mli_bf16* wk,
                                    const mli_bf16* wq, const mli_bf16* wv, float* q_output, int n_batch,
                                    int n_sequence, int emb_dim, void* stream) {
    return mli::launch_latest_paged_bf16(page_table, lengths, wk, wq, wv, q_output, n_batch, n_sequence, emb_dim,
                                         mli::as_stream(stream));
}

int mli_get_latest_k_q_v_paged_rope(void* const* page_table, const int* lengths, const void* wk, const void* wq, const void* wv,
                                    float* q_output, int n_batch, int n_sequence, int emb_dim, int n_heads,
                                    const float* rope_table, int elem, void* stream) {
    return mli::launch_latest_paged_rope(elem, page_table, lengths, wk, wq, wv, q_output, n_batch, n_sequence, emb_dim, n_heads,
                                         rope_table, mli::as_stream(stream));
}

int mli_fill_new_k_v_cache_paged_rope(void* const* page_table, const int* new_batch_idx, const int* lengths, const void* wk,
                                      const void* wv, int n_batch, int n_sequence, int emb_dim, int n_new_items, int n_heads,
                                      const float* rope_table, int elem, void* stream) {
    return mli::launch_fill_paged_rope(elem, nullptr, nullptr, nullptr, page_table, new_batch_idx, lengths, wk, wv, n_batch,
                                       n_sequence, emb_dim, n_new_items, false, 0, 0, n_heads, rope_table,
                                       mli::as_stream(stream));
}

}  // extern "C"

extern "C" {

int mli_prefill(const float* emb_table, const float* wpe, const int* inp, float* inp_embedding, const int* lengths,
                const int* new_item_indices, const float* wk, const float* wv, float* kt_cache, float* v_cache,
                int n_batch, int n_sequence, int input_dim, int output_dim, int n_new_items, void* stream) {
    if (emb_table == nullptr || wpe == nullptr || inp == nullptr) return MLI_ERR_BAD_ARG;
    // wide models: encoder + fill as two launches (see mli_paged_prefill).  The encoder kernel moves float4, so a width
    // that is no multiple of 4 has the prologue form only (its scalar-load instantiation), whatever "prefill_fused" says
    const bool two_launches = !mli::prefill_fuses(input_dim) && input_dim % 4 == 0;
    if (n_new_items > 0) mli::count_launch(two_launches ? mli::kLfPrefillTwoLaunch : mli::kLfPrefillFused);
    if (two_launches) {
        int rc = mli_inference_optimized_encoder(emb_table, wpe, inp, inp_embedding, lengths, new_item_indices, n_batch,
                                                 n_sequence, input_dim, n_new_items, stream);
        if (rc) return rc;
        return mli_fill_new_kt_v_cache(inp_embedding, new_item_indices, lengths, wk, wv, kt_cache, v_cache, n_batch,
                                       n_sequence, input_dim, output_dim, n_new_items, stream);
    }
    return mli::launch_fill_naive_embed(emb_table, wpe, inp, inp_embedding, new_item_indices, lengths, wk, wv, kt_cache,
                                        v_cache, n_batch, n_sequence, input_dim, output_dim, n_new_items,
                                        mli::as_stream(stream));
}

}  // extern "C"
