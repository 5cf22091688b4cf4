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
#include "scan_launch.hpp"
#include "scan_row_order.hpp"

namespace mli {

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

// mli_tune "scan_merge" (lean mode only): 1 (default) = the workgroup that completes a row merges its chunks inside
// the scan launch, 0 = the separate combine launch (bit-identical results)
static thread_local int g_scan_merge = 1;
void set_scan_merge(int v) { g_scan_merge = v != 0; }

// returns 1 when the fused path ran, 0 when the caller should take the three-kernel path, < 0 / > 1 on error
// phases: bit 0 = scan kernel, bit 1 = combine kernel (3 = the whole block; 1 / 2 let bench.py time them apart),
//         bit 2 = lean mode: qkt is neither read nor written (may be null), and with "scan_merge" on there is no
//         combine launch -- the scan merges each row itself (phases 5 then does the whole job, 6 nothing)
// Grid, item size, workspace and LDS: scan_plan.hpp.
template <class E>
static int launch_fused_decode(const float* q, const void* const* page_table, const int* lengths, float* qkt,
                               float* out, int B, int S, int D, void* ws, size_t ws_bytes, hipStream_t st, int phases) {
    const bool lean = (phases & 4) != 0;
    if (lean && g_scan_merge) {
        // chip-filling batches: equal page shares instead of (row, chunk) workgroups (attention_stream.hip); one launch
        // does the whole job, so the "combine only" phase has nothing left to do
        const int r = (phases & 1) ? launch_stream_decode<E>(q, page_table, lengths, out, B, S, D, ws, ws_bytes, st)
                                   : (stream_decode_applies<E>(B, S, D) ? 1 : 0);
        if (r != 0) return r;
    }
    constexpr bool kFp8 = std::is_same<E, ElemFP8>::value;
    const int nj = ceil_div_i(D / E::EPL, kWave);
    if (nj > 8 || D % E::EPL != 0 || S % kPage != 0) return 0;
    if (kFp8 && (!lean || nj > 2)) return 0;   // the fp8 extension: lean form, rows of up to two lane loads (emb_dim <= 2048)
    const ScanVariant v = plain_scan_variant(D, E::EPL);
    const ScanPlan p = plan_chunked_scan(scan_tune(), B, S, S, D, 1, E::kBytes);
    ScanWs w;
    if (!carve_scan_ws(p, ws, ws_bytes, &w)) return 0;
    // lean mode: the in-kernel merge, where the arrival counters can count the rows; otherwise the combine launch
    if (!(lean && g_scan_merge && B <= kMaxArrivalRows)) w.arrivals = nullptr;
    const int ml_per_row = ceil_div_i(S, 64);
    const size_t smem = scan_lds_bytes(p.ct, plain_reduction_bytes(v, E::EPL), plain_merge_stat_bytes(S));
    if (!scan_lds_fits(smem)) return 0;   // rows too long for the statistics' LDS: not applicable, nothing launched
    const auto launch = [&](auto scores) {  // SCORES: the materialising form
        // TBR = rows per load batch: TBR * RPI = 8 token slots for rows of one lane load, 4 for rows of two
        dispatch_scan_variant<E>(v, p.nt, [&](auto NJ, auto DS, auto RPI, auto NT) {
            constexpr bool SC = decltype(scores)::value;
            hipLaunchKernelGGL((fused_decode_scan_kernel<E, NJ(), NT(), (NJ() == 1 ? 8 : 4) / RPI(), DS(), SC, RPI()>),
                               dim3(B, p.grid_y), dim3(kFuThreads), smem, st, q, page_table, lengths, qkt, out, w.ml, w.partial,
                               S, D, p.ct, ml_per_row, p.nchunk, p.direct, w.arrivals);
        });
    };
    if (phases & 1) {
        count_launch(kLfScanChunked);
        if (p.direct) count_launch(p.direct == 2 ? kLfScanRowsOrdered : kLfScanRowsGridOrder);
        if (kFp8 || lean) launch(std::false_type{});
        else if constexpr (!kFp8) launch(std::true_type{});
    }
    int rc = launch_status();
    if (rc) return rc > 0 ? rc + 1 : rc;  // keep 1 free for "ran"
    if (!p.direct && (phases & 2) && w.arrivals == nullptr) {
        // lean: one part per row, no score pass (qkt == nullptr)
        hipLaunchKernelGGL(fused_decode_combine_kernel, dim3(B, lean ? 1 : kCombineParts), dim3(kFuThreads), 0, st, w.ml,
                           w.partial, lengths, lean ? nullptr : qkt, out, S, D, p.ct, ml_per_row, p.nchunk);
        rc = launch_status();
        if (rc) return rc > 0 ? rc + 1 : rc;
    }
    return 1;
}

int launch_fused_decode_elem(int elem, const float* q, const void* const* page_table, const int* lengths, float* qkt,
                             float* out, int B, int S, int D, void* ws, size_t ws_bytes, hipStream_t st, int phases) {
    if (elem == MLI_ELEM_F32) return launch_fused_decode<ElemF32>(q, page_table, lengths, qkt, out, B, S, D, ws, ws_bytes, st, phases);
    if (elem == MLI_ELEM_BF16) return launch_fused_decode<ElemBF16>(q, page_table, lengths, qkt, out, B, S, D, ws, ws_bytes, st, phases);
    return launch_fused_decode<ElemFP8>(q, page_table, lengths, qkt, out, B, S, D, ws, ws_bytes, st, phases);
}

// the materialising compositions (compose.hip); qkt == nullptr selects the lean mode (no scores, in-kernel merge)
int launch_fused_decode_f32(const float* q, const float* const* page_table, const int* lengths, float* qkt, float* out,
                            int B, int S, int D, void* ws, size_t ws_bytes, hipStream_t st) {
    return launch_fused_decode_elem(MLI_ELEM_F32, q, reinterpret_cast<const void* const*>(page_table), lengths, qkt, out, B, S,
                                    D, ws, ws_bytes, st, qkt == nullptr ? 7 : 3);
}

int launch_fused_decode_bf16(const float* q, const uint16_t* const* page_table, const int* lengths, float* qkt,
                             float* out, int B, int S, int D, void* ws, size_t ws_bytes, hipStream_t st) {
    return launch_fused_decode_elem(MLI_ELEM_BF16, q, reinterpret_cast<const void* const*>(page_table), lengths, qkt, out, B, S,
                                    D, ws, ws_bytes, st, qkt == nullptr ? 7 : 3);
}

}  // namespace mli

extern "C" int mli_decode_scan_paged(const float* q_output, const void* const* page_table, const int* lengths,
                                     float* qkt_output, float* attention_result, int n_batch, int n_sequence,
                                     int emb_dim, int elem_bf16, int phases, void* workspace, size_t workspace_bytes,
                                     void* stream) {
    if (phases < 1 || phases > 7 || phases == 4) return MLI_ERR_BAD_ARG;
    if (!(phases & 4) && qkt_output == nullptr) return MLI_ERR_BAD_ARG;
    hipStream_t st = mli::as_stream(stream);
    if (elem_bf16 < MLI_ELEM_F32 || elem_bf16 > MLI_ELEM_FP8) return MLI_ERR_BAD_ARG;
    if (elem_bf16 == MLI_ELEM_FP8 && !(phases & 4)) return MLI_ERR_BAD_ARG;   // the fp8 extension has the lean form only
    if (phases == 7)   // the whole lean job
        return mli::launch_lean_scan(q_output, page_table, lengths, attention_result, n_batch, n_sequence, emb_dim, 1, 1,
                                     0, 0, elem_bf16, workspace, workspace_bytes, st);
    const mli::WsBody body = mli::ws_body(workspace, workspace_bytes);
    // not applicable: shape not covered by the single-pass kernel (emb_dim too wide) or no workspace
    return mli::fused_status(mli::launch_fused_decode_elem(elem_bf16, q_output, page_table, lengths, qkt_output, attention_result,
                                                          n_batch, n_sequence, emb_dim, body.ptr, body.bytes, st, phases));
}

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
