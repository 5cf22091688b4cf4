// Single-pass decode attention over paged KV ("flash-decoding" form) used by the paged_attention compositions:
// every page is visited ONCE and both its K rows and its V rows are consumed in that visit, with an online
// (running max / running sum) softmax per wave.  Compared with the separate q.K^T and softmax.V passes this halves
// the number of page visits (one TLB / DRAM-page walk per 2/3 of a block instead of per 1/3 -- pages are scattered
// over the pool), removes the softmax launch and keeps the scores out of the critical path.
//
// The reference's contract for the composition (src/kernels/paged_attention.cu:358-377) is kept: on return
// qkt_output holds the masked softmax probabilities with a zero tail, attention_result holds sum p.V, rows with
// length 0 give zeros.  Raw scores are written by the scan kernel; the combine kernel merges the per-chunk
// (max, sum, partial output) triples in chunk order and normalises the row.
//
//   scan    grid = (B, chunks) rows fast (XCD balance), 256 threads; a wave owns whole pages
//   combine grid = B, 256 threads
#include "scan_item_body.hpp"
#include "scan_row_order.hpp"

namespace mli {

int sv_chunk_tokens_for(int n_batch, int n_sequence);  // attention_scan.hip
int tuned_chunk_tokens();
template <class E>
int launch_stream_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                         void* ws, size_t ws_bytes, hipStream_t st);   // attention_stream.hip
template <class E>
bool stream_decode_applies(int B, int S, int D);
size_t stats_region_bytes_for(int B, int S);
int nt_loads_for(int B, int S, int D, int esize);

template <class E, int NJ, bool NT, int TBR, bool DS, bool SCORES, int RPI>
__global__ __launch_bounds__(kFuThreads, 2) void fused_decode_scan_kernel(
    const float* __restrict__ q, const void* const* __restrict__ page_table, const int* __restrict__ lengths,
    float* __restrict__ qkt, float* __restrict__ out, float2* ml, float* partial,
    int S, int D, int ct, int ml_per_row, int nchunk_max, int direct, unsigned* arrivals) {
    extern __shared__ __align__(16) unsigned char smem_raw[];
    // Which (row, chunk) this workgroup takes follows from its grid position.  Workgroups are dealt to the 8 XCDs
    // round-robin by linear grid position, i.e. by blockIdx.x % 8 (n_batch is a multiple of 8 in every configuration
    // that fills the chip).  Rotating the row index by the chunk index spreads the chunks of one row over the XCDs, so
    // every XCD streams a mix of all rows instead of a fixed eighth of them whose total length differs from the
    // others' by +-10 % (tools/scan_trace.py: XCDs done at 615 .. 701 us).
    const int c = blockIdx.y;
    int b = (int)((blockIdx.x + (unsigned)c) % gridDim.x);
    if (direct == 2) b = longest_first_row(lengths, (int)gridDim.x, S, (int)blockIdx.x);
    fused_scan_item<E, NJ, NT, TBR, DS, SCORES, RPI>(q, page_table, lengths, qkt, out, ml, partial, S, D, ct, ml_per_row,
                                                     nchunk_max, direct, arrivals, b, c, c == 0, (int)gridDim.x, smem_raw);
}

// grid = (B, kCombineParts).  Every part merges the row's chunk statistics (cheap, identical result), part 0 also
// writes attention_result; each part turns its slice of the raw scores into probabilities (zero tail included).
constexpr int kCombineParts = 4;

__global__ __launch_bounds__(kFuThreads) void fused_decode_combine_kernel(
    const float2* __restrict__ ml, const float* __restrict__ partial, const int* __restrict__ lengths,
    float* __restrict__ qkt, float* __restrict__ out, int S, int D, int ct, int ml_per_row, int nchunk) {
    const int b = blockIdx.x;
    const int part = blockIdx.y;
    const int L = min(lengths[b], S);
    const int nc = (L + ct - 1) / ct;
    float* qkt_row = qkt + (int64_t)b * S;
    const int per = ((S + kCombineParts - 1) / kCombineParts + 3) & ~3;
    const int i0 = part * per, i1 = min(S, i0 + per);
    if (nc == 0) {
        if (qkt != nullptr) for (int i = i0 + threadIdx.x; i < i1; i += kFuThreads) qkt_row[i] = 0.f;
        if (part == 0) for (int i = threadIdx.x; i < D; i += kFuThreads) out[(int64_t)b * D + i] = 0.f;
        return;
    }
    const float2* row = ml + (int64_t)b * ml_per_row;
    float m = -INFINITY;
    for (int i = 0; i < nc; ++i) m = fmaxf(m, row[i].x);
    float l = 0.f;
    for (int i = 0; i < nc; ++i) l = fmaf(row[i].y, expf(row[i].x - m), l);
    const float inv_l = 1.f / l;
    if (part == 0) {
        const float* pr = partial + (int64_t)b * nchunk * D;
        for (int d = threadIdx.x; d < D; d += kFuThreads) {
            float r = 0.f;
            for (int i = 0; i < nc; ++i) r = fmaf(pr[(int64_t)i * D + d], expf(row[i].x - m), r);
            out[(int64_t)b * D + d] = r * inv_l;
        }
    }
    if (qkt == nullptr) return;  // lean mode: the scores were never written
    for (int i = i0 + threadIdx.x; i < i1; i += kFuThreads) qkt_row[i] = i < L ? expf(qkt_row[i] - m) * inv_l : 0.f;
}

static thread_local int g_row_order = 1;  // mli_tune "scan_row_order": 0 = one-workgroup-per-row grids take the rows in grid order
void set_row_order(int v) { g_row_order = v != 0; }
int scan_row_order() { return g_row_order; }   // attention_heads.hip
// mli_tune "scan_merge" (lean mode only): 1 (default) = the workgroup that completes a row merges its chunks inside
// the scan launch, 0 = the separate combine launch (bit-identical results)
static thread_local int g_scan_merge = 1;
void set_scan_merge(int v) { g_scan_merge = v != 0; }

// Tokens per workgroup of the single-pass scan: the largest power of two <= 512 that still cuts the batch into
// >= 2048 (row, chunk) slots, i.e. with ragged lengths about two rounds of real items for the 512 workgroups the chip
// holds.  Measured: B=1024, S=4096 -> 512 (256: +2.4 %, 1024: +1 % with ragged lengths); B=256, S=1024 -> 128 (round 2,
// scan launch: 46.9 us against 49.6 at 256 and 54.3 at 512, where 384 items of very unequal size cannot even fill the
// 512 slots once; lean form 52.5 / 53.1 / 56.2).
int fused_chunk_tokens(int B, int S) {   // (also attention_heads.hip)
    if (tuned_chunk_tokens() != 0) return sv_chunk_tokens_for(B, S);  // forced (mli_tune)
    int ct = 512;
    while (ct > 64 && (int64_t)B * ceil_div_i(S, ct) < 2048) ct >>= 1;
    return ct;
}

// returns 1 when the fused path ran, 0 when the caller should take the three-kernel path, < 0 / > 1 on error
// phases: bit 0 = scan kernel, bit 1 = combine kernel (3 = the whole block; 1 / 2 let bench.py time them apart),
//         bit 2 = lean mode: qkt is neither read nor written (may be null), and with "scan_merge" on there is no
//         combine launch -- the scan merges each row itself (phases 5 then does the whole job, 6 nothing)
template <class E>
static int launch_fused_decode(const float* q, const void* const* page_table, const int* lengths, float* qkt,
                               float* out, int B, int S, int D, void* ws, size_t ws_bytes, hipStream_t st,
                               int phases = 3) {
    const bool lean = (phases & 4) != 0;
    if (lean && g_scan_merge) {
        // chip-filling batches: equal page shares instead of (row, chunk) workgroups (attention_stream.hip); one launch
        // does the whole job, so the "combine only" phase has nothing left to do
        const int r = (phases & 1) ? launch_stream_decode<E>(q, page_table, lengths, out, B, S, D, ws, ws_bytes, st)
                                   : (stream_decode_applies<E>(B, S, D) ? 1 : 0);
        if (r != 0) return r;
    }
    const int Du = D / E::EPL;
    const int nj = ceil_div_i(Du, kWave);
    if (nj > 8 || D % E::EPL != 0 || S % kPage != 0) return 0;
    constexpr bool kFp8 = std::is_same<E, ElemFP8>::value;
    if (kFp8 && (!lean || nj > 2)) return 0;   // the fp8 extension: lean form, rows of up to two lane loads (emb_dim <= 2048)
    // fp8 rows narrower than one load instruction: 2 or 4 token slots per instruction (scan_common.hpp)
    const int rpi = kFp8 ? (Du <= 16 ? 4 : Du <= 32 ? 2 : 1) : 1;
    const bool dsplit = nj > 2;  // wide rows: the four waves split the row instead of the pages
    const int nj_ds = ceil_div_i(Du, kWave * kFuWaves);  // 1 or 2
    // short sequences with a full batch: one workgroup per row (no partials, no combine launch) beats two 64-token
    // chunks (README workload, S = 128: 200 vs 209 us)
    const int ct = (S <= 128 && B >= 256 && tuned_chunk_tokens() == 0) ? 128 : fused_chunk_tokens(B, S);
    const int nchunk = ceil_div_i(S, ct);
    // one workgroup per row: hand the rows out longest first where the batch has more rows than the chip has workgroup slots
    const bool ordered = g_row_order && nchunk == 1 && B > 512 && B <= kMaxOrderedRows && S / kPage <= kMaxOrderedPages;
    const int direct = nchunk == 1 ? (ordered ? 2 : 1) : 0;
    const size_t stats_bytes = stats_region_bytes_for(B, S);
    float2* ml = nullptr;
    float* partial = nullptr;
    if (!direct) {
        if (ws == nullptr || ws_bytes < stats_bytes + (size_t)B * nchunk * D * sizeof(float)) return 0;
        ml = reinterpret_cast<float2*>(ws);
        partial = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + stats_bytes);
    }
    const int ml_per_row = ceil_div_i(S, 64);
    // lean mode: arrival counters (one per row, zero between launches) in front of the workspace body
    unsigned* arrivals = nullptr;
    if (lean && !direct && g_scan_merge && B <= kMaxArrivalRows) arrivals = ws_arrivals(ws);  // ws != nullptr: checked above
    // page pointers of the chunk | reduction buffer (also holds the row's chunk statistics during the in-kernel merge)
    const size_t red_bytes = (dsplit ? (size_t)2 * kFuWaves * 16 : (size_t)kFuWaves * nj * (kWave / rpi) * E::EPL) * sizeof(float);
    const size_t stat_bytes_row = (size_t)ml_per_row * 8;  // upper bound of the triples a row can have
    const size_t smem = (size_t)(ct / kPage) * 8 + (red_bytes > stat_bytes_row ? red_bytes : stat_bytes_row);
    // several chunks per row: grid rows 0 .. nchunk-1 run the full chunks, grid row nchunk every row's remainder as one
    // item (fused_scan_item)
    const dim3 grid(B, direct ? 1 : nchunk + 1);
    const bool nt = nt_loads_for(B, S, D, E::kBytes);
    // TBR = rows per load batch: TBR * RPI = 8 token slots for rows of one lane load, 4 for rows of two
#define MLI_FU_LAUNCH(NJ, DS, SCORES, RPI)                                                                                \
    do {                                                                                                                 \
        if (nt)                                                                                                          \
            hipLaunchKernelGGL((fused_decode_scan_kernel<E, NJ, true, (NJ == 1 ? 8 : 4) / RPI, DS, SCORES, RPI>), grid,  \
                               dim3(kFuThreads), smem, st, q, page_table, lengths, qkt, out, ml, partial, S, D, ct,      \
                               ml_per_row, nchunk, direct, arrivals);                                                     \
        else                                                                                                             \
            hipLaunchKernelGGL((fused_decode_scan_kernel<E, NJ, false, (NJ == 1 ? 8 : 4) / RPI, DS, SCORES, RPI>), grid, \
                               dim3(kFuThreads), smem, st, q, page_table, lengths, qkt, out, ml, partial, S, D, ct,      \
                               ml_per_row, nchunk, direct, arrivals);                                                     \
    } while (0)
    if constexpr (kFp8) {
        if (phases & 1) {
            if (rpi == 4) MLI_FU_LAUNCH(1, false, false, 4);
            else if (rpi == 2) MLI_FU_LAUNCH(1, false, false, 2);
            else if (nj == 1) MLI_FU_LAUNCH(1, false, false, 1);
            else MLI_FU_LAUNCH(2, false, false, 1);
        }
    } else if (phases & 1) {
        const auto launch = [&](auto scores) {  // SCORES: the materialising form
            constexpr bool SC = decltype(scores)::value;
            if (dsplit) {
                if (nj_ds == 1) MLI_FU_LAUNCH(1, true, SC, 1);
                else MLI_FU_LAUNCH(2, true, SC, 1);
            } else if (nj == 1) {
                MLI_FU_LAUNCH(1, false, SC, 1);
            } else {
                MLI_FU_LAUNCH(2, false, SC, 1);
            }
        };
        if (lean) launch(std::false_type{});
        else launch(std::true_type{});
    }
#undef MLI_FU_LAUNCH
    int rc = launch_status();
    if (rc) return rc > 0 ? rc + 1 : rc;  // keep 1 free for "ran"
    if (!direct && (phases & 2) && arrivals == nullptr) {
        // lean: one part per row, no score pass (qkt == nullptr)
        hipLaunchKernelGGL(fused_decode_combine_kernel, dim3(B, lean ? 1 : kCombineParts), dim3(kFuThreads), 0, st, ml,
                           partial, lengths, lean ? nullptr : qkt, out, S, D, ct, ml_per_row, nchunk);
        rc = launch_status();
        if (rc) return rc > 0 ? rc + 1 : rc;
    }
    return 1;
}

// qkt == nullptr selects the lean mode (no scores, in-kernel merge)
int launch_fused_decode_f32(const float* q, const float* const* page_table, const int* lengths, float* qkt, float* out,
                            int B, int S, int D, void* ws, size_t ws_bytes, hipStream_t st) {
    return launch_fused_decode<ElemF32>(q, reinterpret_cast<const void* const*>(page_table), lengths, qkt, out, B, S, D,
                                        ws, ws_bytes, st, qkt == nullptr ? 7 : 3);
}

int launch_fused_decode_bf16(const float* q, const uint16_t* const* page_table, const int* lengths, float* qkt,
                             float* out, int B, int S, int D, void* ws, size_t ws_bytes, hipStream_t st) {
    return launch_fused_decode<ElemBF16>(q, reinterpret_cast<const void* const*>(page_table), lengths, qkt, out, B, S, D,
                                         ws, ws_bytes, st, qkt == nullptr ? 7 : 3);
}

// fp8 (OCP e4m3) pages: the lean form only
int launch_fused_decode_fp8(const float* q, const uint8_t* const* page_table, const int* lengths, float* out, int B, int S,
                            int D, void* ws, size_t ws_bytes, hipStream_t st) {
    return launch_fused_decode<ElemFP8>(q, reinterpret_cast<const void* const*>(page_table), lengths, nullptr, out, B, S, D, ws,
                                        ws_bytes, st, 7);
}

}  // namespace mli

extern "C" int mli_decode_scan_paged(const float* q_output, const void* const* page_table, const int* lengths,
                                     float* qkt_output, float* attention_result, int n_batch, int n_sequence,
                                     int emb_dim, int elem_bf16, int phases, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    { const mli::WsBody body = mli::ws_body(workspace, workspace_bytes); workspace = body.ptr; workspace_bytes = body.bytes; }
    if (phases < 1 || phases > 7 || phases == 4) return MLI_ERR_BAD_ARG;
    if (!(phases & 4) && qkt_output == nullptr) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    if (elem_bf16 < MLI_ELEM_F32 || elem_bf16 > MLI_ELEM_FP8) return MLI_ERR_BAD_ARG;
    if (elem_bf16 == MLI_ELEM_FP8 && !(phases & 4)) return MLI_ERR_BAD_ARG;   // the fp8 extension has the lean form only
    const int r = elem_bf16 == MLI_ELEM_FP8
                      ? mli::launch_fused_decode<mli::ElemFP8>(q_output, page_table, lengths, qkt_output, attention_result,
                                                               n_batch, n_sequence, emb_dim, workspace, workspace_bytes, st, phases)
                  : elem_bf16 ? mli::launch_fused_decode<mli::ElemBF16>(q_output, page_table, lengths, qkt_output,
                                                                      attention_result, n_batch, n_sequence, emb_dim,
                                                                      workspace, workspace_bytes, st, phases)
                            : mli::launch_fused_decode<mli::ElemF32>(q_output, page_table, lengths, qkt_output,
                                                                     attention_result, n_batch, n_sequence, emb_dim,
                                                                     workspace, workspace_bytes, st, phases);
    if (r == 1) return 0;
    if (r == 0) return MLI_ERR_BAD_ARG;  // shape not covered by the single-pass kernel (emb_dim too wide) or no workspace
    return r < 0 ? r : r - 1;
}

namespace mli {

}  // namespace mli

#ifdef MLI_SCAN_TRACE
extern "C" int mli_debug_scan_trace(unsigned long long* host, int n_slots) {
    if (n_slots > mli::kTraceSlots) n_slots = mli::kTraceSlots;
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(mli::mli_scan_trace), (size_t)n_slots * 8 * sizeof(unsigned long long));
}
extern "C" int mli_debug_scan_trace_clear(void) {
    void* p = nullptr;
    hipError_t e = hipGetSymbolAddress(&p, HIP_SYMBOL(mli::mli_scan_trace));
    if (e != hipSuccess) return (int)e;
    return (int)hipMemset(p, 0, sizeof(unsigned long long) * mli::kTraceSlots * 8);
}
#endif
