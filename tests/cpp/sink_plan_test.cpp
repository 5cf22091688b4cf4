// The launch plan of the paged scan with attention sinks (min_llm_inference_amd/csrc/scan_plan.hpp: sink_span,
// lean_scan_kind, and plan_chunked_scan at that span) against values worked out by hand, CPU only: the header is plain
// C++ and is compiled here without HIP.  The shapes are those of tests/test_sinks_scan_gpu.py.
#include <cstdio>
#include <initializer_list>

#include "scan_plan.hpp"

using namespace mli;

namespace {

int failures = 0;

#define CHECK_EQ(what, got, want)                                                                       \
    do {                                                                                                \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                  \
        if (g_ != w_) {                                                                                 \
            std::printf("[FAIL] %s: %s = %lld, expected %lld\n", label, what, g_, w_);                   \
            ++failures;                                                                                 \
        }                                                                                               \
    } while (0)

struct Row {
    int chunk_tokens;              // mli_tune "chunk_tokens" (scan_row_order 1, nt_loads 2)
    int elem, B, S, D, H, W, K;    // MLI_ELEM_*
    int span;                      // 16 * (ceil(K / 16) + ceil(W / 16) + 1), at most S
    int ct, nchunk, direct, grid_y;
    size_t body_bytes;             // B * ceil(S / 64) * H * 8 rounded up to 256, + B * nchunk * D * 4
};

// By hand from the rules in scan_plan.hpp's comments: the item size is 128 for span <= 128 with B >= 256, else the largest
// power of two in 64 .. 512 with B * ceil(span / ct) >= 2048 (64 if none); one item per row is direct, ranked (2) for
// 512 < B <= 2048.
const Row kRows[] = {
    {0, 0, 40, 64, 64, 1, 5, 1, /**/ 48, 64, 1, 1, 1, 512 + 40 * 1 * 64 * 4},
    {0, 1, 40, 64, 64, 2, 16, 4, /**/ 48, 64, 1, 1, 1, 768 + 40 * 1 * 64 * 4},
    {0, 2, 40, 64, 64, 1, 17, 16, /**/ 64, 64, 1, 1, 1, 512 + 40 * 1 * 64 * 4},
    {0, 0, 40, 64, 64, 2, 8, 17, /**/ 64, 64, 1, 1, 1, 768 + 40 * 1 * 64 * 4},
    {0, 0, 40, 64, 64, 1, 33, 20, /**/ 64, 64, 1, 1, 1, 512 + 40 * 1 * 64 * 4},
    {0, 0, 24, 256, 512, 1, 40, 4, /**/ 80, 64, 2, 0, 3, 768 + 24 * 2 * 512 * 4},
    {0, 1, 24, 256, 512, 8, 100, 20, /**/ 160, 64, 3, 0, 4, 6144 + 24 * 3 * 512 * 4},
    {256, 2, 24, 256, 512, 1, 100, 20, /**/ 160, 256, 1, 1, 1, 768 + 24 * 1 * 512 * 4},
    {0, 0, 20, 1024, 256, 2, 513, 4, /**/ 560, 64, 9, 0, 10, 5120 + 20 * 9 * 256 * 4},
    {0, 1, 24, 512, 1024, 8, 130, 4, /**/ 176, 64, 3, 0, 4, 12288 + 24 * 3 * 1024 * 4},
    {0, 2, 8, 256, 2048, 1, 100, 4, /**/ 144, 64, 3, 0, 4, 256 + 8 * 3 * 2048 * 4},
    {0, 0, 700, 128, 64, 1, 50, 4, /**/ 96, 128, 1, 2, 1, 11264 + 700 * 1 * 64 * 4},
    {0, 0, 700, 128, 64, 2, 50, 4, /**/ 96, 128, 1, 2, 1, 22528 + 700 * 1 * 64 * 4},
};

}  // namespace

int main() {
    int rows = 0;
    for (const Row& r : kRows) {
        char label[128];
        std::snprintf(label, sizeof label, "elem %d B %d S %d D %d H %d W %d K %d chunk_tokens %d", r.elem, r.B, r.S, r.D, r.H,
                      r.W, r.K, r.chunk_tokens);
        const ScanTune tune{r.chunk_tokens, 1, 2};
        const int esize = r.elem == MLI_ELEM_FP8 ? 1 : r.elem == MLI_ELEM_BF16 ? 2 : 4;
        CHECK_EQ("window_shape_supported", window_shape_supported(r.B, r.S, r.D, r.H, r.elem), 1);
        CHECK_EQ("lean_scan_kind", lean_scan_kind(r.S, r.W, r.K), kScanSinks);
        CHECK_EQ("sink_span", sink_span(r.S, r.W, r.K), r.span);
        const ScanPlan p = plan_chunked_scan(tune, r.B, r.S, r.span, r.D, r.H, esize);
        CHECK_EQ("ct", p.ct, r.ct);
        CHECK_EQ("nchunk", p.nchunk, r.nchunk);
        CHECK_EQ("direct", p.direct, r.direct);
        CHECK_EQ("grid_y", p.grid_y, r.grid_y);
        CHECK_EQ("body_bytes", p.body_bytes, r.body_bytes);
        // the workspace is the un-windowed one of the same (B, S, D, H): a span never has more items than ceil(S / 64) ...
        const ScanPlan plain = plan_chunked_scan(tune, r.B, r.S, r.S, r.D, r.H, esize);
        CHECK_EQ("stats_bytes", p.stats_bytes, plain.stats_bytes);
        CHECK_EQ("items within the row stride", p.nchunk <= plan_ceil_div(r.S, 64), 1);
        // ... and never more than the plain scan's worst case, B * ceil(S / 64) partial rows
        CHECK_EQ("body within the plain workspace",
                 p.body_bytes <= plain.stats_bytes + (size_t)r.B * plan_ceil_div(r.S, 64) * r.D * sizeof(float), 1);
        // K = 0 is the windowed scan (whose launcher asks for window_span), K + W >= S (and W >= S) the plain one
        CHECK_EQ("K 0: kind", lean_scan_kind(r.S, r.W, 0), kScanWindow);
        CHECK_EQ("one more sink page never shrinks the span", sink_span(r.S, r.W, r.K) >= window_span(r.S, r.W), 1);
        for (int k : {r.S - r.W, r.S - r.W + 1, r.S, 1 << 30}) {
            CHECK_EQ("K + W >= S: kind", lean_scan_kind(r.S, r.W, k), kScanPlain);
            CHECK_EQ("K + W >= S: the span would be the row", sink_span(r.S, r.W, k), r.S);
        }
        CHECK_EQ("K + W = S - 1: kind", lean_scan_kind(r.S, r.W, r.S - r.W - 1), kScanSinks);
        for (int w : {r.S, r.S + 1, 0, -1}) CHECK_EQ("no window: kind", lean_scan_kind(r.S, w, r.K), kScanPlain);
        ++rows;
    }
    {
        const char* label = "sink_span";
        CHECK_EQ("(1024, 1, 1)", sink_span(1024, 1, 1), 48);
        CHECK_EQ("(1024, 16, 16)", sink_span(1024, 16, 16), 48);
        CHECK_EQ("(1024, 17, 16)", sink_span(1024, 17, 16), 64);
        CHECK_EQ("(1024, 17, 17)", sink_span(1024, 17, 17), 80);
        CHECK_EQ("(1024, 1000, 4)", sink_span(1024, 1000, 4), 1024);
        CHECK_EQ("(1 << 30, 1 << 29, 1 << 29)", sink_span(1 << 30, 1 << 29, 1 << 29), 1 << 30);   // no overflow
        // a span covers every virtual row: L - 16 * skip <= span for every L
        for (int S : {64, 256, 1024})
            for (int W = 1; W < S; W += 7)
                for (int K = 1; K + W < S; K += 5)
                    for (int L = 0; L <= S; ++L) {
                        const int lo = L > W ? L - W : 0, ps = plan_ceil_div(K, 16);
                        const int skip = lo / 16 > ps ? lo / 16 - ps : 0;
                        if (L - 16 * skip > sink_span(S, W, K)) {
                            std::printf("[FAIL] S %d W %d K %d L %d: the virtual row exceeds the span\n", S, W, K, L);
                            ++failures;
                        }
                    }
    }
    std::printf("%d sink plan rows, %d failure(s)\n", rows, failures);
    return failures != 0;
}
