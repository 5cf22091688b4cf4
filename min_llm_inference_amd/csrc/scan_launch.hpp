// The HIP side of the chunked paged scans' launch plan (scan_plan.hpp): the workspace carve, the kernel-variant dispatch,
// and the host functions the scan files and the compositions call across files.
#pragma once

#include <type_traits>

#include "launch_count.hpp"
#include "scan_item_body.hpp"
#include "scan_plan.hpp"

namespace mli {

static_assert(kPlanPage == kPage && kPlanWave == kWave && kPlanWaves == kFuWaves && kPlanMaxRows == kMaxArrivalRows,
              "scan_plan.hpp mirrors the device constants");

// ---- across files ----------------------------------------------------------------------------------------------------
ScanTune scan_tune();                                   // attention_scan.hip: the calling thread's mli_tune values
int nt_loads_for(int B, int S, int D, int esize);       // nt_loads_rule under the calling thread's "nt_loads"
// attention_stream.hip: equal page shares instead of (row, item) workgroups; 1 = ran, 0 = not applicable, else an error
// (+1 if positive)
template <class E>
int launch_stream_decode(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                         void* ws, size_t ws_bytes, hipStream_t st);
template <class E>
bool stream_decode_applies(int B, int S, int D);
// attention_fused.hip, over the workspace BODY (ws_body) and an element type its caller has accepted: 1 = ran, 0 = not
// applicable (rows too wide, or no workspace), else an error (+1 if positive)
int launch_fused_decode_elem(int elem, const float* q, const void* const* page_table, const int* lengths, float* qkt,
                             float* out, int B, int S, int D, void* ws, size_t ws_bytes, hipStream_t st, int phases);
// compose.hip: the lean scan for (n_heads, n_kv_heads, window, n_sink) -- n_kv_heads == n_heads: no grouping; window <= 0
// or >= n_sequence: none; n_sink 0, or n_sink + window >= n_sequence: no sinks, or no gap they could bridge -- over the
// caller's WHOLE workspace; returns a C ABI status.  It holds the one check of head counts and shape (MLI_ERR_BAD_ARG before
// any launch) and picks the kernel family: the plain single-head scan above, the single-head scan under a window
// (attention_window.hpp) or the multi-head scan (attention_heads.hpp).
// launch_lean_attention: launch_fill_and_latest, then that scan over q_output.
int launch_lean_scan(const float* q, const void* const* page_table, const int* lengths, float* out, int B, int S, int D,
                     int n_heads, int n_kv_heads, int window, int n_sink, int elem, void* workspace, size_t workspace_bytes,
                     hipStream_t st);
int launch_lean_attention(int elem, void* const* page_table, const int* lengths, const void* wk, const void* wq,
                          const void* wv, const int* new_batch_idx, float* q_output, float* out, int B, int S, int D,
                          int n_new_items, int n_heads, int n_kv_heads, int window, int n_sink, void* workspace,
                          size_t workspace_bytes, hipStream_t st);

// launch_fused_decode_elem's protocol as a C ABI status: "not applicable" is a bad argument
inline int fused_status(int r) { return r == 1 ? 0 : r == 0 ? MLI_ERR_BAD_ARG : r < 0 ? r : r - 1; }

// ---- workspace carve -------------------------------------------------------------------------------------------------
struct ScanWs {
    float2* ml;          // (m, l) statistics
    float* partial;      // partial output rows
    unsigned* arrivals;  // row arrival counters, in front of the body
};
// false: the plan needs a body the caller did not give (what that returns is the caller's business).  A plan of one
// workgroup per row needs none: all null.
inline bool carve_scan_ws(const ScanPlan& p, void* ws, size_t ws_bytes, ScanWs* w) {
    *w = ScanWs{nullptr, nullptr, nullptr};
    if (p.direct) return true;
    if (ws == nullptr || ws_bytes < p.body_bytes) return false;
    w->ml = reinterpret_cast<float2*>(ws);
    w->partial = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + p.stats_bytes);
    w->arrivals = ws_arrivals(ws);
    return true;
}

// ---- kernel variant --------------------------------------------------------------------------------------------------
// Calls f(NJ, DS, RPI, NT) with std::integral_constants; f names the kernel.  fp8 pages have four variants only (rows of
// up to two lane loads, no D-split), everything else has no RPI: nothing else is instantiated.
template <class E, class F>
inline void dispatch_scan_variant(const ScanVariant& v, bool nt, F&& f) {
    using std::integral_constant;
    const auto go = [&](auto nj, auto ds, auto rpi) {
        if (nt) f(nj, ds, rpi, std::true_type{});
        else f(nj, ds, rpi, std::false_type{});
    };
    if constexpr (std::is_same<E, ElemFP8>::value) {
        if (v.rpi == 4) go(integral_constant<int, 1>{}, std::false_type{}, integral_constant<int, 4>{});
        else if (v.rpi == 2) go(integral_constant<int, 1>{}, std::false_type{}, integral_constant<int, 2>{});
        else if (v.nj == 1) go(integral_constant<int, 1>{}, std::false_type{}, integral_constant<int, 1>{});
        else go(integral_constant<int, 2>{}, std::false_type{}, integral_constant<int, 1>{});
    } else if (v.ds) {
        if (v.nj == 1) go(integral_constant<int, 1>{}, std::true_type{}, integral_constant<int, 1>{});
        else go(integral_constant<int, 2>{}, std::true_type{}, integral_constant<int, 1>{});
    } else {
        if (v.nj == 1) go(integral_constant<int, 1>{}, std::false_type{}, integral_constant<int, 1>{});
        else go(integral_constant<int, 2>{}, std::false_type{}, integral_constant<int, 1>{});
    }
}

}  // namespace mli
