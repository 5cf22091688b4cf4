// The launch plan of the chunked paged scans (min_llm_inference_amd/csrc/scan_plan.hpp) against a table of expected values,
// CPU only: the header is plain C++ and is compiled here without HIP.
#include <cstdio>

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
    ScanTune tune;                 // chunk_tokens, scan_row_order, nt_loads
    int elem, B, S, D, H, W;       // MLI_ELEM_*; W 0 = no window
    int ct, nchunk, direct, grid_y;
    size_t body_bytes, lds_bytes;
    int NJ, DS, RPI, nt;
};

// The expected values were NOT computed with scan_plan.hpp: they are the output of a throw-away program that pasted the
// launch arithmetic of the commit before the header existed (launch_fused_decode, launch_heads_decode, launch_window_decode,
// launch_window_heads with fused_chunk_tokens, heads_chunk_tokens, heads_stats_bytes, stats_region_bytes, window_span and
// nt_loads_for) and printed one line per input.
const Row kRows[] = {
    {{0, 1, 2}, 0, 256, 128, 256, 1, 0, /**/ 128, 1, 1, 1, 266240, 4160, 1, 0, 1, 0},   // one 128-token item per row
    {{0, 1, 2}, 0, 1024, 128, 2048, 1, 0, /**/ 128, 1, 2, 1, 8404992, 576, 2, 1, 1, 1},   // longest first (README workload)
    {{0, 1, 2}, 0, 512, 128, 256, 1, 0, /**/ 128, 1, 1, 1, 532480, 4160, 1, 0, 1, 0},   // B 512: grid order
    {{0, 1, 2}, 0, 2048, 128, 256, 1, 0, /**/ 128, 1, 2, 1, 2129920, 4160, 1, 0, 1, 0},   // B 2048: the last batch ranked
    {{0, 1, 2}, 0, 2049, 128, 256, 1, 0, /**/ 128, 1, 1, 1, 2131200, 4160, 1, 0, 1, 0},   // B 2049: grid order
    {{0, 1, 2}, 0, 256, 1024, 256, 1, 0, /**/ 128, 8, 0, 9, 2129920, 4160, 1, 0, 1, 0},   // 128-token items
    {{0, 1, 2}, 0, 1024, 4096, 256, 1, 0, /**/ 512, 8, 0, 9, 8912896, 4352, 1, 0, 1, 1},   // 512-token items, non-temporal by working set
    {{0, 1, 2}, 0, 8, 4096, 256, 1, 0, /**/ 64, 64, 0, 65, 528384, 4128, 1, 0, 1, 0},   // 64-token items
    {{0, 1, 2}, 0, 8, 128, 256, 1, 0, /**/ 64, 2, 0, 3, 16640, 4128, 1, 0, 1, 0},   // small batch, short rows: two 64-token items
    {{0, 1, 2}, 0, 8, 64, 256, 1, 0, /**/ 64, 1, 1, 1, 8448, 4128, 1, 0, 1, 0},   // one item per row, few rows
    {{0, 1, 2}, 0, 600, 1040, 256, 1, 0, /**/ 256, 5, 0, 6, 3153664, 4224, 1, 0, 1, 1},   // S no multiple of the item size
    {{256, 1, 2}, 0, 256, 1024, 256, 1, 0, /**/ 256, 4, 0, 5, 1081344, 4224, 1, 0, 1, 0},   // chunk_tokens 256
    {{256, 1, 2}, 0, 256, 128, 256, 1, 0, /**/ 256, 1, 1, 1, 266240, 4224, 1, 0, 1, 0},   // chunk_tokens 256 over short rows: one item, not the 128 rule
    {{256, 1, 2}, 0, 1024, 256, 256, 1, 0, /**/ 256, 1, 2, 1, 1081344, 4224, 1, 0, 1, 0},   // chunk_tokens 256 = S: longest first
    {{0, 0, 2}, 0, 1024, 128, 256, 1, 0, /**/ 128, 1, 1, 1, 1064960, 4160, 1, 0, 1, 0},   // scan_row_order 0
    {{0, 1, 0}, 0, 1024, 4096, 256, 1, 0, /**/ 512, 8, 0, 9, 8912896, 4352, 1, 0, 1, 0},   // nt_loads 0
    {{0, 1, 1}, 0, 8, 64, 256, 1, 0, /**/ 64, 1, 1, 1, 8448, 4128, 1, 0, 1, 1},   // nt_loads 1
    {{0, 1, 2}, 0, 8, 1024, 128, 1, 1, /**/ 64, 1, 1, 1, 5120, 4128, 1, 0, 1, 0},   // W 1: span 32
    {{0, 1, 2}, 0, 8, 1024, 128, 1, 16, /**/ 64, 1, 1, 1, 5120, 4128, 1, 0, 1, 0},   // W 16: span 32
    {{0, 1, 2}, 0, 8, 1024, 128, 1, 17, /**/ 64, 1, 1, 1, 5120, 4128, 1, 0, 1, 0},   // W 17: span 48
    {{0, 1, 2}, 0, 8, 1024, 128, 1, 1000, /**/ 64, 16, 0, 17, 66560, 4128, 1, 0, 1, 0},   // W 1000: span S
    {{0, 1, 2}, 0, 8, 4096, 128, 1, 1024, /**/ 64, 17, 0, 18, 73728, 4128, 1, 0, 1, 0},   // windowed, several items
    {{0, 1, 2}, 0, 1024, 4096, 256, 1, 100, /**/ 128, 1, 2, 1, 1572864, 4160, 1, 0, 1, 0},   // windowed, longest first: S / 16 beyond the ranked pages, the span within
    {{0, 1, 2}, 0, 1024, 4096, 256, 1, 1020, /**/ 512, 3, 0, 4, 3670016, 4352, 1, 0, 1, 1},   // windowed: span / 16 = 65 beyond the ranked pages
    {{0, 1, 2}, 1, 8, 1024, 4096, 1, 256, /**/ 64, 5, 0, 6, 656384, 544, 2, 1, 1, 0},   // windowed bf16 D-split
    {{0, 1, 2}, 2, 8, 1024, 512, 1, 256, /**/ 64, 5, 0, 6, 82944, 8224, 1, 0, 2, 0},   // windowed fp8, two slots per instruction
    {{0, 1, 2}, 0, 8, 1024, 128, 2, 256, /**/ 64, 5, 0, 6, 22528, 6176, 1, 0, 1, 0},   // windowed, two heads
    {{0, 1, 2}, 1, 2, 16384, 1024, 32, 8192, /**/ 128, 65, 0, 66, 663552, 20544, 2, 0, 1, 0},   // windowed, 32 heads: item size raised
    {{0, 1, 2}, 0, 1024, 4096, 256, 4, 100, /**/ 128, 1, 2, 1, 3145728, 6208, 1, 0, 1, 0},   // windowed heads, longest first
    {{0, 1, 2}, 1, 2, 16384, 1024, 32, 0, /**/ 128, 128, 0, 129, 1179648, 32832, 2, 0, 1, 0},   // 32 heads: item size raised
    {{0, 1, 2}, 0, 8, 1024, 128, 2, 0, /**/ 64, 16, 0, 17, 67584, 6176, 1, 0, 1, 0},   // two heads
    {{0, 1, 2}, 0, 1024, 128, 512, 8, 0, /**/ 128, 1, 2, 1, 2228224, 12352, 2, 0, 1, 0},   // heads, longest first, rows of two lane loads
    {{0, 1, 2}, 1, 256, 128, 1024, 8, 0, /**/ 128, 1, 1, 1, 1081344, 20544, 2, 0, 1, 0},   // bf16 heads, rows of two lane loads
    {{0, 1, 2}, 0, 8, 1024, 256, 1, 0, /**/ 64, 16, 0, 17, 132096, 4128, 1, 0, 1, 0},   // fp32 D 256
    {{0, 1, 2}, 0, 8, 1024, 512, 1, 0, /**/ 64, 16, 0, 17, 263168, 8224, 2, 0, 1, 0},   // fp32 D 512
    {{0, 1, 2}, 0, 8, 1024, 516, 1, 0, /**/ 64, 16, 0, 17, 265216, 544, 1, 1, 1, 0},   // fp32 D 516
    {{0, 1, 2}, 0, 8, 1024, 1024, 1, 0, /**/ 64, 16, 0, 17, 525312, 544, 1, 1, 1, 0},   // fp32 D 1024
    {{0, 1, 2}, 0, 8, 1024, 2048, 1, 0, /**/ 64, 16, 0, 17, 1049600, 544, 2, 1, 1, 0},   // fp32 D 2048
    {{0, 1, 2}, 1, 8, 1024, 512, 1, 0, /**/ 64, 16, 0, 17, 263168, 8224, 1, 0, 1, 0},   // bf16 D 512
    {{0, 1, 2}, 1, 8, 1024, 1024, 1, 0, /**/ 64, 16, 0, 17, 525312, 16416, 2, 0, 1, 0},   // bf16 D 1024
    {{0, 1, 2}, 1, 8, 1024, 4096, 1, 0, /**/ 64, 16, 0, 17, 2098176, 544, 2, 1, 1, 0},   // bf16 D 4096
    {{0, 1, 2}, 2, 8, 1024, 256, 1, 0, /**/ 64, 16, 0, 17, 132096, 4128, 1, 0, 4, 0},   // fp8 D 256
    {{0, 1, 2}, 2, 8, 1024, 512, 1, 0, /**/ 64, 16, 0, 17, 263168, 8224, 1, 0, 2, 0},   // fp8 D 512
    {{0, 1, 2}, 2, 8, 1024, 1024, 1, 0, /**/ 64, 16, 0, 17, 525312, 16416, 1, 0, 1, 0},   // fp8 D 1024
    {{0, 1, 2}, 2, 8, 1024, 2048, 1, 0, /**/ 64, 16, 0, 17, 1049600, 32800, 2, 0, 1, 0},   // fp8 D 2048
    {{0, 1, 2}, 0, 8, 16384, 1024, 1, 0, /**/ 64, 256, 0, 257, 8404992, 2080, 1, 1, 1, 1},   // D-split, long rows: the per-64-token statistics bound exceeds the reduction buffer
    {{0, 1, 2}, 0, 8, 16384, 1024, 1, 8192, /**/ 64, 129, 0, 130, 4243456, 1064, 1, 1, 1, 0},   // the same under a window: the per-item bound does
};

void check_row(const Row& r, const char* label) {
    const int epl = r.elem == MLI_ELEM_FP8 ? 16 : r.elem == MLI_ELEM_BF16 ? 8 : 4;
    const int span = r.W ? window_span(r.S, r.W) : r.S;
    const ScanPlan p = plan_chunked_scan(r.tune, r.B, r.S, span, r.D, r.H, 16 / epl);
    ScanVariant v = plain_scan_variant(r.D, epl);
    size_t lds;
    if (r.H > 1) {   // the multi-head launchers: rows of one or two lane loads, whole pages per wave
        v = ScanVariant{plan_ceil_div(r.D / epl, 64), false, 1};
        lds = scan_lds_bytes(p.ct, heads_reduction_bytes(v.nj, epl), heads_merge_stat_bytes(p.nchunk, r.H));
    } else {
        lds = scan_lds_bytes(p.ct, plain_reduction_bytes(v, epl),
                             r.W ? window_merge_stat_bytes(p.nchunk) : plain_merge_stat_bytes(r.S));
    }
    CHECK_EQ("ct", p.ct, r.ct);
    CHECK_EQ("nchunk", p.nchunk, r.nchunk);
    CHECK_EQ("direct", p.direct, r.direct);
    CHECK_EQ("grid.y", p.grid_y, r.grid_y);
    CHECK_EQ("body bytes", p.body_bytes, r.body_bytes);
    CHECK_EQ("LDS bytes", lds, r.lds_bytes);
    CHECK_EQ("NJ", v.nj, r.NJ);
    CHECK_EQ("DS", v.ds, r.DS);
    CHECK_EQ("RPI", v.rpi, r.RPI);
    CHECK_EQ("nt", p.nt, r.nt);
}

struct Shape {
    const char* what;
    int B, S, D, H, elem;
};
// tests/test_heads_abi.py: BAD
const Shape kBadHeads[] = {{"emb_dim % H", 8, 64, 128, 3, 0},        {"head_dim 16", 8, 64, 128, 8, 0},
                           {"head_dim 512", 8, 64, 1024, 2, 1},      {"fp8 pages", 8, 64, 512, 8, 2},
                           {"fp32 emb_dim 1024", 8, 64, 1024, 8, 0}, {"bf16 emb_dim 2048", 8, 64, 2048, 8, 1},
                           {"n_sequence % 16", 8, 72, 128, 2, 0},    {"n_batch > 16384", 16385, 64, 128, 2, 0},
                           {"n_heads 0", 8, 64, 128, 0, 0},          {"too many items x heads", 2, 131088, 1024, 32, 1}};
// tests/test_window_abi.py: BAD_PLAIN
const Shape kBadPlain[] = {{"n_sequence % 16", 8, 72, 128, 1, 0},     {"n_sequence % 16 bf16", 8, 40, 128, 1, 1},
                           {"n_sequence % 16 fp8", 8, 72, 128, 1, 2}, {"n_batch 16385", 16385, 64, 128, 1, 0},
                           {"n_batch 16385 bf16", 16385, 64, 128, 1, 1}, {"n_batch 0", 0, 64, 128, 1, 0},
                           {"fp32 emb_dim 2052", 8, 64, 2052, 1, 0},  {"bf16 emb_dim 4104", 8, 64, 4104, 1, 1},
                           {"bf16 emb_dim % 8", 8, 64, 132, 1, 1},    {"fp8 emb_dim % 16", 8, 64, 136, 1, 2},
                           {"fp8 emb_dim 2064", 8, 64, 2064, 1, 2},   {"element type 3", 8, 64, 128, 1, 3}};
// hd / elements per lane load: lanes per head
const struct { Shape s; int lg; } kGoodHeads[] = {{{"fp32 hd 64", 8, 64, 128, 2, 0}, 4},    {{"fp32 hd 32", 8, 64, 128, 4, 0}, 3},
                                                  {{"bf16 hd 32", 8, 64, 128, 4, 1}, 2},    {{"bf16 hd 256", 8, 64, 1024, 4, 1}, 5},
                                                  {{"fp32 hd 256", 16384, 16, 512, 2, 0}, 6}, {{"bf16 hd 32 x 32", 2, 131072, 1024, 32, 1}, 2}};
const Shape kGoodPlain[] = {{"fp32 emb_dim 2048", 8, 64, 2048, 1, 0}, {"bf16 emb_dim 4096", 8, 64, 4096, 1, 1},
                            {"fp8 emb_dim 2048", 16384, 16, 2048, 1, 2}, {"fp32 emb_dim 4", 1, 16, 4, 1, 0}};

}  // namespace

int main() {
    for (const Row& r : kRows) {
        char label[160];
        std::snprintf(label, sizeof label, "tune (%d, %d, %d) elem %d B %d S %d D %d H %d W %d", r.tune.chunk_tokens,
                      r.tune.row_order, r.tune.nt_loads, r.elem, r.B, r.S, r.D, r.H, r.W);
        check_row(r, label);
    }
    {
        const char* label = "window_span";
        CHECK_EQ("W 1", window_span(1024, 1), 32);
        CHECK_EQ("W 16", window_span(1024, 16), 32);
        CHECK_EQ("W 17", window_span(1024, 17), 48);
        CHECK_EQ("W 1000", window_span(1024, 1000), 1024);
        CHECK_EQ("W 1024 of 4096", window_span(4096, 1024), 1040);
    }
    for (const Shape& s : kBadHeads) {
        const char* label = s.what;
        CHECK_EQ("heads_lanes_log2", heads_lanes_log2(s.B, s.S, s.D, s.H, s.elem), -1);
        CHECK_EQ("heads_shape_supported", heads_shape_supported(s.B, s.S, s.D, s.H, s.elem), 0);
        CHECK_EQ("window_shape_supported", window_shape_supported(s.B, s.S, s.D, s.H, s.elem), 0);
    }
    for (const Shape& s : kBadPlain) {
        const char* label = s.what;
        CHECK_EQ("window_plain_shape_ok", window_plain_shape_ok(s.B, s.S, s.D, s.elem), 0);
        CHECK_EQ("window_shape_supported", window_shape_supported(s.B, s.S, s.D, s.H, s.elem), 0);
    }
    for (const auto& g : kGoodHeads) {
        const char* label = g.s.what;
        CHECK_EQ("heads_lanes_log2", heads_lanes_log2(g.s.B, g.s.S, g.s.D, g.s.H, g.s.elem), g.lg);
        CHECK_EQ("window_shape_supported", window_shape_supported(g.s.B, g.s.S, g.s.D, g.s.H, g.s.elem), 1);
    }
    for (const Shape& s : kGoodPlain) {
        const char* label = s.what;
        CHECK_EQ("window_plain_shape_ok", window_plain_shape_ok(s.B, s.S, s.D, s.elem), 1);
    }
    const int n = (int)(sizeof kRows / sizeof kRows[0]);
    std::printf("%d plan rows, %d failure(s)\n", n, failures);
    return failures ? 1 : 0;
}
