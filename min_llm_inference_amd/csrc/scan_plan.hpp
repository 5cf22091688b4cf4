// The launch plan of the chunked paged scans -- the single-head scan (attention_fused.hip), its forms under a sliding
// window, with or without sinks (attention_window.hpp), and the multi-head scan, plain, windowed, with sinks and with
// grouped-query attention (attention_heads.hpp): every rule that decides how such a scan is launched, once.  Plain C++ over int /
// size_t / bool, no HIP types and no global state (tests/cpp/scan_plan_test.cpp compiles it alone); the mli_tune values the
// rules depend on come in as a ScanTune.
#pragma once

#include <cstddef>

#include "mli_kernels.h"

namespace mli {

// device_common.hpp / scan_item_body.hpp: kPage, kWave, kFuWaves, kMaxArrivalRows (scan_launch.hpp holds them equal)
constexpr int kPlanPage = MLI_PAGE_BLOCK_SIZE;
constexpr int kPlanWave = 64;
constexpr int kPlanWaves = 4;
constexpr int kPlanMaxRows = 16384;

constexpr int kMaxOrderedRows = 2048;   // longest-first row order (scan_row_order.hpp): rows it can rank ...
constexpr int kMaxOrderedPages = 64;    // ... and live pages per row its histogram covers
constexpr int kMaxItemTokens = 1024;
constexpr int kMaxMergeStats = 4096;    // float2 entries: the 32 KiB of LDS the last arriver stages a row's statistics in

inline int plan_ceil_div(int a, int b) { return (a + b - 1) / b; }

// The calling thread's mli_tune values (scan_tune(), attention_scan.hip)
struct ScanTune {
    int chunk_tokens;   // "chunk_tokens": 0 = the heuristic, else the forced item size (what sv_chunk_tokens_for then returns)
    int row_order;      // "scan_row_order": 0 = one-workgroup-per-row grids take the rows in grid order
    int nt_loads;       // "nt_loads": 0 = default cache policy, 1 = non-temporal, 2 = by working set
};

// K/V loads: non-temporal where the rows' K/V (upper bound B * S * D * e * 2 bytes) is far beyond the 256 MiB
// Infinity Cache -- every byte is read once per step and nothing survives to the next one --, default policy where a
// good part of it can stay on-die between two steps.  Measured (lean scan, fp32, D=256, S=1024, lengths U[S/4, 3S/4]):
// B=128 / 256: default policy 6 / 5 % faster; B=512 / 1024 / 2048: non-temporal 6 / 11 / 10 % faster.
inline bool nt_loads_rule(int setting, int B, int S, int D, int esize) {
    if (setting != 2) return setting != 0;
    return (long long)B * S * D * esize * 2 > ((long long)768 << 20);
}

// The resident slice of the equal-shares scan (attention_stream.hip, mli_tune "scan_resident_mib").  Where the K/V stream is
// non-temporal, a fixed slice of the pages, sized to fit the Infinity Cache, is loaded with the default policy instead and
// stays on die from one decode step to the next (tools/membench.hip `resident`: non-temporal loads leave such lines alone).
// Both functions are constexpr so that the kernel and a host program (tests/cpp/scan_resident_test.cpp) compile this text.
//   resident_threshold: the share of the launch's K/V bytes that resident_mib MiB are, as a value in 0 .. 65536.
//   page_kv_bytes = 2 * 16 * D * e (the x segment of a page is not read by the scan); 64-bit throughout (2048 rows x 256
//   pages x 64 KiB = 2^35 bytes at the largest shape the kernel takes).
constexpr unsigned resident_threshold(long long total_pages, long long page_kv_bytes, int resident_mib) {
    if (resident_mib <= 0) return 0u;
    if (total_pages <= 0 || page_kv_bytes <= 0) return 65536u;
    const unsigned long long t = (((unsigned long long)resident_mib << 20) * 65536ull) /
                                 ((unsigned long long)total_pages * (unsigned long long)page_kv_bytes);
    return t > 65536ull ? 65536u : (unsigned)t;
}
//   resident_keeps: whether a page belongs to the slice.  A multiplicative hash of the page's address (4-KiB granularity)
//   against the threshold: the same page gets the same answer in every step, whatever the partition, the row's length or
//   the batch's composition, and as the threshold falls (the batch grows) pages only leave the slice.
constexpr bool resident_keeps(unsigned long long page_ptr, unsigned thr) {
    return (((unsigned)(page_ptr >> 12) * 2654435761u) >> 16) < thr;
}

// The tokens a windowed row can span: its window plus the part of the first live page below it, whole pages
// (1 <= window < S: the entry points hand everything else on).
inline int window_span(int S, int window) {
    const long long span = (long long)kPlanPage * (plan_ceil_div(window, kPlanPage) + 1);
    return span < S ? (int)span : S;
}

// ... and with n_sink sink tokens in front (1 <= n_sink, n_sink + window < S): the sink pages, the window's pages and the
// part of the window's first page below it -- the longest virtual row (scan_item_body.hpp, SINK).
inline int sink_span(int S, int window, int n_sink) {
    const long long span = (long long)kPlanPage * (plan_ceil_div(n_sink, kPlanPage) + plan_ceil_div(window, kPlanPage) + 1);
    return span < S ? (int)span : S;
}

// Which scan a lean call with (window, n_sink) is -- the hand-offs of the entry points, once: no window (<= 0, or >=
// n_sequence) is the plain scan whatever n_sink; no sinks is the windowed scan; sinks and window that together cover
// n_sequence leave no row a gap and are the plain scan again.
enum ScanKind { kScanPlain, kScanWindow, kScanSinks };
inline ScanKind lean_scan_kind(int S, int window, int n_sink) {
    if (window <= 0 || window >= S) return kScanPlain;
    if (n_sink <= 0) return kScanWindow;
    return (long long)n_sink + window >= S ? kScanPlain : kScanSinks;
}

// Tokens per item over rows of `span` tokens (n_sequence, or the span a window leaves).
//   Short sequences with a full batch: one workgroup per row (no partials, no combine launch) beats two 64-token chunks
//   (README workload, S = 128: 200 vs 209 us).
//   Otherwise the largest power of two <= 512 that still cuts the batch into >= 2048 (row, item) slots, i.e. with ragged
//   lengths about two rounds of real items for the 512 workgroups the chip holds.  Measured: B=1024, S=4096 -> 512 (256:
//   +2.4 %, 1024: +1 % with ragged lengths); B=256, S=1024 -> 128 (round 2, scan launch: 46.9 us against 49.6 at 256 and 54.3
//   at 512, where 384 items of very unequal size cannot even fill the 512 slots once; lean form 52.5 / 53.1 / 56.2).
//   Several heads: raised where a row's (items x heads) statistics would not fit the LDS the last arriver stages them in
//   (n_sequence 16384 with 32 heads and a small batch); a size exists for every shape heads_lanes_log2 accepts.
inline int scan_item_tokens(const ScanTune& t, int B, int span, int H) {
    int ct;
    if (t.chunk_tokens != 0) {
        ct = t.chunk_tokens;
    } else if (span <= 128 && B >= 256) {
        ct = 128;
    } else {
        ct = 512;
        while (ct > 64 && (long long)B * plan_ceil_div(span, ct) < 2048) ct >>= 1;
    }
    if (H > 1)
        while (ct < kMaxItemTokens && (long long)plan_ceil_div(span, ct) * H > kMaxMergeStats) ct <<= 1;
    return ct;
}

// Workspace body = [(m, l) per row, 64 tokens and head: B * ceil(S / 64) * H float2, 256-B aligned][partial rows].  The row
// stride is n_sequence's whatever the item size or the window: calls of different shapes share one layout.
inline size_t scan_stats_bytes(int B, int S, int H = 1) {
    const size_t n = (size_t)B * plan_ceil_div(S, 64) * H * 8;
    return (n + 255) & ~(size_t)255;
}

struct ScanPlan {
    int ct;              // tokens per item
    int nchunk;          // items a row can have
    int direct;          // 0 = several items per row, 1 = one workgroup per row in grid order, 2 = ... longest row first
    int grid_y;          // grid = (B, grid_y): rows 0 .. nchunk-1 run the full items, row nchunk every row's remainder
    size_t stats_bytes;  // the statistics region in front of the partial rows
    size_t body_bytes;   // what the workspace body must hold unless direct
    bool nt;             // non-temporal K/V loads
};

// S = n_sequence; span = S, window_span(S, window) or sink_span(S, window, n_sink); esize = bytes per page element.
// D_read = the columns of a K / V segment the scan reads: D, or with grouped-query attention n_kv_heads * head_dim --
// the working set the cache policy is judged by.  Everything else follows D: the output and the partial rows are D wide.
inline ScanPlan plan_chunked_scan(const ScanTune& t, int B, int S, int span, int D, int D_read, int H, int esize) {
    ScanPlan p;
    p.ct = scan_item_tokens(t, B, span, H);
    p.nchunk = plan_ceil_div(span, p.ct);
    // one workgroup per row: hand the rows out longest first where the batch has more rows than the chip has workgroup slots
    const bool ordered = t.row_order && p.nchunk == 1 && B > 512 && B <= kMaxOrderedRows && span / kPlanPage <= kMaxOrderedPages;
    p.direct = p.nchunk == 1 ? (ordered ? 2 : 1) : 0;
    p.grid_y = p.direct ? 1 : p.nchunk + 1;
    p.stats_bytes = scan_stats_bytes(B, S, H);
    p.body_bytes = p.stats_bytes + (size_t)B * p.nchunk * D * sizeof(float);
    p.nt = nt_loads_rule(t.nt_loads, B, span, D_read, esize);
    return p;
}
// every K / V column read: the scans without grouped-query attention
inline ScanPlan plan_chunked_scan(const ScanTune& t, int B, int S, int span, int D, int H, int esize) {
    return plan_chunked_scan(t, B, S, span, D, D, H, esize);
}

// The single-head kernel variant.  epl = elements per 16-byte lane load: 4 (fp32), 8 (bf16), 16 (fp8).
struct ScanVariant {
    int nj;    // template NJ: lane loads per row and wave, 1 or 2
    bool ds;   // D-split (rows of more than two lane loads): the four waves split the row instead of the pages
    int rpi;   // token slots per load instruction: fp8 rows narrower than one instruction take 2 or 4 (scan_common.hpp)
};
inline ScanVariant plain_scan_variant(int D, int epl) {
    const int Du = D / epl;
    const int nj = plan_ceil_div(Du, kPlanWave);
    ScanVariant v;
    v.ds = nj > 2;
    v.nj = v.ds ? plan_ceil_div(Du, kPlanWave * kPlanWaves) : nj;
    v.rpi = epl == 16 ? (Du <= 16 ? 4 : Du <= 32 ? 2 : 1) : 1;
    return v;
}

// Dynamic LDS of a workgroup: the item's page pointers | the reduction buffer, which also holds the row's statistics
// during the in-kernel merge (so the larger of the two).
inline size_t scan_lds_bytes(int ct, size_t reduction_bytes, size_t merge_stat_bytes) {
    return (size_t)(ct / kPlanPage) * 8 + (reduction_bytes > merge_stat_bytes ? reduction_bytes : merge_stat_bytes);
}
// What a launch gets without raising the kernel's dynamic-LDS limit: 64 KiB for static and dynamic LDS together.  The scan
// kernels' static part (wave statistics, the row-order histogram, a flag) is 312 bytes at most; 512 are set aside.  A plan
// beyond it is refused before anything is launched: the merge statistics grow with n_sequence (single head: 8 bytes per 64
// tokens, i.e. n_sequence 519936 at items of 64; under a window: 8 bytes per item of the span).
constexpr size_t kLaunchLdsLimit = 64 * 1024;
constexpr size_t kScanStaticLds = 512;
inline bool scan_lds_fits(size_t dynamic_bytes) { return dynamic_bytes + kScanStaticLds <= kLaunchLdsLimit; }
// single head: the waves' partial output rows, or with the D-split two buffers of the 16 partial scores of a page
inline size_t plain_reduction_bytes(const ScanVariant& v, int epl) {
    return (v.ds ? (size_t)2 * kPlanWaves * 16 : (size_t)kPlanWaves * v.nj * (kPlanWave / v.rpi) * epl) * sizeof(float);
}
// several heads: the waves' parked rows and (m, l) pairs
inline size_t heads_reduction_bytes(int nj, int epl) {
    return (size_t)kPlanWaves * nj * kPlanWave * (epl * sizeof(float) + 8);
}
// The merge statistics' bound is a different expression in each launcher; each sets the dynamic LDS of existing launches
// and stays as it is.
// Single head, no window: one pair per 64 tokens of n_sequence -- the workspace's row stride, an upper bound at every item
// size; the merge stages one pair per item, so nchunk pairs would do, and why the stride was taken cannot be told from the code.
inline size_t plain_merge_stat_bytes(int S) { return (size_t)plan_ceil_div(S, 64) * 8; }
// Single head, window: one pair per item of the span -- what the merge stages.
inline size_t window_merge_stat_bytes(int nchunk) { return (size_t)nchunk * 8; }
// Several heads, with or without a window: one pair per (item, head) -- what the merge stages; scan_item_tokens keeps it
// within kMaxMergeStats.
inline size_t heads_merge_stat_bytes(int nchunk, int H) { return (size_t)nchunk * H * 8; }

// ---- shapes the scans take (everything else is MLI_ERR_BAD_ARG before anything is launched) -------------------------------
// Several heads: log2 of the lanes per head, or -1.
inline int heads_lanes_log2(int B, int S, int D, int H, int elem) {
    if (B <= 0 || B > kPlanMaxRows || S <= 0 || S % kPlanPage != 0 || D <= 0 || H < 1 || D % H != 0) return -1;
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return -1;
    const int hd = D / H;
    if (hd != 32 && hd != 64 && hd != 128 && hd != 256) return -1;
    const int epl = elem == MLI_ELEM_BF16 ? 8 : 4;
    if (D / epl > 2 * kPlanWave) return -1;   // rows of at most two lane loads: whole pages per wave
    // the last arriver stages a row's (items x heads) statistics in LDS: even at the largest item size they must fit
    if ((long long)plan_ceil_div(S, kMaxItemTokens) * H > kMaxMergeStats) return -1;
    int lg = 0;
    while ((epl << lg) < hd) ++lg;
    return lg;
}
inline int heads_shape_supported(int n_batch, int n_sequence, int emb_dim, int n_heads, int elem) {
    return heads_lanes_log2(n_batch, n_sequence, emb_dim, n_heads, elem) >= 0;
}
// One head under a window: what the lean chunked scan takes, with the rows the arrival counters can count.
inline bool window_plain_shape_ok(int B, int S, int D, int elem) {
    if (B <= 0 || B > kPlanMaxRows || S <= 0 || S % kPlanPage != 0 || D <= 0) return false;
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16 && elem != MLI_ELEM_FP8) return false;
    const int epl = elem == MLI_ELEM_FP8 ? 16 : elem == MLI_ELEM_BF16 ? 8 : 4;
    if (D % epl != 0) return false;
    const int nj = plan_ceil_div(D / epl, kPlanWave);
    return elem == MLI_ELEM_FP8 ? nj <= 2 : nj <= 8;
}
inline int window_shape_supported(int n_batch, int n_sequence, int emb_dim, int n_heads, int elem) {
    if (n_heads < 1) return 0;
    return n_heads == 1 ? window_plain_shape_ok(n_batch, n_sequence, emb_dim, elem)
                        : heads_lanes_log2(n_batch, n_sequence, emb_dim, n_heads, elem) >= 0;
}

// ---- grouped-query attention (attention_heads.hpp, GQA) -----------------------------------------------------------------------
// n_kv_heads K/V heads serve n_heads query heads, g = n_heads / n_kv_heads (any integer) consecutive query heads each: query
// head h attends K/V head h / g, which owns columns [(h / g) * hd, (h / g + 1) * hd) of the K and V segments.  The shapes
// are the multi-head scan's, with or without a window.
inline int gqa_shape_supported(int n_batch, int n_sequence, int emb_dim, int n_heads, int n_kv_heads, int elem) {
    if (n_heads <= 1 || !window_shape_supported(n_batch, n_sequence, emb_dim, n_heads, elem)) return 0;
    return n_kv_heads >= 1 && n_kv_heads <= n_heads && n_heads % n_kv_heads == 0;
}
// The lane map.  A lane's 16-byte unit u lies in query head u >> lg (heads_item_body.hpp: a head is a group of G = 1 << lg
// lanes); the unit it LOADS from a K or V segment is the same position inside K/V head (u >> lg) / g:
//   kvu = (u / G / g) * G + u % G,   0 <= kvu < n_kv_heads * G = Dkv / EPL;   g = 1: kvu = u.
// constexpr, so that the kernel and a host program (tests/cpp/gqa_map_test.cpp) compile this text.
constexpr int gqa_kv_unit(int u, int lg, int g) { return (((u >> lg) / g) << lg) + (u & ((1 << lg) - 1)); }

// ---- the causal multi-query prompt scan (attention_prompt.hpp) --------------------------------------------------------------
// What it takes: fp32 and bf16 pages with rows of at most two lane loads -- one head: fp32 to emb_dim 512, bf16 to 1024;
// several heads, with or without grouped K/V heads: what heads_lanes_log2 / gqa_shape_supported accept.  n_kv_heads ==
// n_heads: no grouping.  Everything else, fp8 pages included, is refused before any launch.
inline bool prompt_scan_shape_ok(int B, int S, int D, int H, int Hkv, int elem) {
    if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return false;
    if (H < 1 || Hkv < 1 || Hkv > H) return false;
    if (H == 1) {
        if (!window_plain_shape_ok(B, S, D, elem)) return false;
        const int epl = elem == MLI_ELEM_BF16 ? 8 : 4;
        return plan_ceil_div(D / epl, kPlanWave) <= 2;
    }
    if (Hkv == H) return heads_lanes_log2(B, S, D, H, elem) >= 0;
    return gqa_shape_supported(B, S, D, H, Hkv, elem) != 0;
}
// TQ, the consecutive query positions a workgroup of the prompt scan shares every K / V load among: a compile-time constant
// per kernel variant (element type, lane loads per row, one head or several), the largest of 8 / 4 / 2 that compiles without
// scratch (DESIGN 3.6d has the register table).  constexpr: the kernel's template argument and mli_prompt_scan_tq are this text.
constexpr int prompt_scan_tq(int epl, int nj, bool heads) {
    if (heads) return (epl == 4 ? 8 : 4) / nj;   // fp32: 8 / 4 for rows of one / two lane loads; bf16: 4 / 2
    return epl == 8 && nj == 2 ? 4 : 8;
}
// The grid: n_seg * ceil(max_count / TQ) workgroups of 256 threads in x.  The HIP runtime launches fewer than 2^32 work items
// per grid dimension (hip_runtime_api.h, hipModuleLaunchKernel: "gridDim.x * blockDim.x ... always less than 2^32"), that is
// at most 2^24 - 1 workgroups; a larger call is refused with the other shapes, before any pointer is looked at.
inline bool prompt_scan_grid_ok(int n_seg, int max_count, int tq) {
    return (long long)n_seg * plan_ceil_div(max_count, tq) * (kPlanWaves * kPlanWave) < (1LL << 32);
}

}  // namespace mli
