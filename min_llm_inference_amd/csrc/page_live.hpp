// Which pages of a row are live under a sliding window with attention sinks -- the one rule the windowed prefill
// (proj_gemm*.hip, encoder_decoder.hip) and a host scheduler that returns pages early share.  Plain C++ over int,
// constexpr, no HIP types (tests/cpp/page_release_test.cpp compiles it alone, as scan_plan.hpp's resident_threshold).
//
// A row of n tokens, window W, n_sink = K, with 1 <= W, 0 <= K and K + W < S (kScanWindow / kScanSinks of lean_scan_kind):
//   lo = max(0, n - W), p0 = lo / 16, ps = ceil(K / 16), skip = max(0, p0 - ps)      (fused_scan_item / heads_scan_item)
//   page i is DEAD at n iff ps <= i < p0: no scan of a row of n or more tokens reads one of its slots (p0 is monotone in n,
//   so a page dead at n is dead at every n' >= n).
//   live tokens, in order: [0, 16 ps) u [16 p0, n) when skip > 0, else [0, n) -- n - 16 skip of them; live index s' is slot
//   s' < 16 ps ? s' : s' + 16 skip (the virtual row of sink_page, scan_item_body.hpp).
#pragma once

namespace mli {

// MLI_PAGE_BLOCK_SIZE / PAGE_BLOCK_SIZE; no include, so that the host scheduler's sources reach this file by its relative
// path alone (gemm_common.hpp and paged_item_storage.cpp hold the three equal)
constexpr int kLivePage = 16;

constexpr int live_ceil_div(int a, int b) { return (a + b - 1) / b; }
constexpr int live_sink_pages(int n_sink) { return n_sink > 0 ? live_ceil_div(n_sink, kLivePage) : 0; }                // ps
constexpr int live_window_page(int n, int window) { return n > window ? (n - window) / kLivePage : 0; }                // p0
constexpr int live_skip_pages(int n, int window, int n_sink) {                                                       // skip
    return live_window_page(n, window) > live_sink_pages(n_sink) ? live_window_page(n, window) - live_sink_pages(n_sink) : 0;
}
constexpr bool page_dead(int page, int n, int window, int n_sink) {
    return page >= live_sink_pages(n_sink) && page < live_window_page(n, window);
}
constexpr int live_tokens(int n, int window, int n_sink) { return n - kLivePage * live_skip_pages(n, window, n_sink); }
// live index (0 <= live < live_tokens) -> token slot
constexpr int live_slot(int live, int n, int window, int n_sink) {
    return live < kLivePage * live_sink_pages(n_sink) ? live : live + kLivePage * live_skip_pages(n, window, n_sink);
}
// The pages a row of n tokens holds so that positions [0, n + ahead) are covered: the indices in [0, ceil((n + ahead) / 16))
// that are not dead at n (row_pages = the table's width caps the range).
constexpr int live_pages_covering(int n, int ahead, int window, int n_sink, int row_pages) {
    const int top = live_ceil_div(n + ahead, kLivePage) < row_pages ? live_ceil_div(n + ahead, kLivePage) : row_pages;
    const int ps = live_sink_pages(n_sink) < top ? live_sink_pages(n_sink) : top;
    const int p0 = live_window_page(n, window) < top ? live_window_page(n, window) : top;
    return p0 > ps ? top - (p0 - ps) : top;
}
// ... and its upper bound over all n: the sink pages, the pages of window + look-ahead, and the part of the window's first
// page below it.  (top - p0 <= ceil((n + ahead) / 16) - floor((n - window) / 16) <= ceil((window + ahead) / 16) + 1.)
constexpr int live_pages_bound(int ahead, int window, int n_sink) {
    return live_sink_pages(n_sink) + live_ceil_div(window + ahead, kLivePage) + 1;
}
// The most live tokens a prefilled row can have: the sink pages, the window, and the part of the window's first page
// below it (at most 15 tokens) -- never more than the row.
constexpr int live_tokens_bound(int S, int window, int n_sink) {
    return kLivePage * live_sink_pages(n_sink) + window + kLivePage - 1 < S ? kLivePage * live_sink_pages(n_sink) + window + kLivePage - 1 : S;
}

}  // namespace mli
