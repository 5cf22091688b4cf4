// Grouped-query attention in the launch plan (min_llm_inference_amd/csrc/scan_plan.hpp), CPU only: the header is plain C++
// and is compiled here without HIP.
//   - the lane map gqa_kv_unit, the text the kernel compiles, by enumeration over every supported (elem, D, H, Hkv);
//   - gqa_shape_supported against a table of accepted and refused shapes;
//   - plan_chunked_scan with read width D against the plan without a read width, field by field, and what a narrower read
//     width may change (the cache policy) and may not (everything else).
#include <cstdio>
#include <initializer_list>

#include "scan_plan.hpp"

using namespace mli;

namespace {

int failures = 0;

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::printf("[FAIL] " __VA_ARGS__);   \
            std::printf(": %s\n", #cond);         \
            ++failures;                           \
        }                                         \
    } while (0)

// every (elem, D, H, Hkv) the scan takes at a small (B, S): the lane map is checked unit by unit
int check_lane_map() {
    int shapes = 0;
    for (int elem : {MLI_ELEM_F32, MLI_ELEM_BF16}) {
        const int epl = elem == MLI_ELEM_BF16 ? 8 : 4;
        for (int hd : {32, 64, 128, 256}) {
            for (int H = 2; H * hd <= 1024; ++H) {
                const int D = H * hd;
                const int lg = heads_lanes_log2(8, 64, D, H, elem);
                for (int Hkv = 1; Hkv <= H; ++Hkv) {
                    const bool ok = gqa_shape_supported(8, 64, D, H, Hkv, elem);
                    CHECK(ok == (lg >= 0 && H % Hkv == 0), "elem %d D %d H %d Hkv %d", elem, D, H, Hkv);
                    if (!ok) continue;
                    ++shapes;
                    const int G = 1 << lg, g = H / Hkv, Du = D / epl, Dkvu = Hkv * hd / epl;
                    CHECK(G * epl == hd && Du <= 2 * kPlanWave, "elem %d D %d H %d: lanes per head", elem, D, H);
                    for (int u = 0; u < Du; ++u) {
                        const int kvu = gqa_kv_unit(u, lg, g);
                        const int h = u / G;
                        CHECK(kvu >= 0 && kvu < Dkvu, "elem %d D %d H %d Hkv %d u %d: kvu %d", elem, D, H, Hkv, u, kvu);
                        CHECK(kvu == (u / G / g) * G + u % G, "elem %d D %d H %d Hkv %d u %d: kvu %d", elem, D, H, Hkv, u, kvu);
                        // the units of query head h are the consecutive units of K/V head h / g, in order
                        CHECK(kvu / G == h / g && kvu % G == u % G, "elem %d D %d H %d Hkv %d u %d: kvu %d", elem, D, H, Hkv, u, kvu);
                        if (u % G != 0) CHECK(kvu == gqa_kv_unit(u - 1, lg, g) + 1, "elem %d D %d H %d Hkv %d u %d", elem, D, H, Hkv, u);
                        // bytes: the loaded columns are those of K/V head h / g, element for element
                        CHECK(kvu * epl == (h / g) * hd + (u % G) * epl, "elem %d D %d H %d Hkv %d u %d", elem, D, H, Hkv, u);
                        if (g == 1) CHECK(kvu == u, "g = 1 is the identity: elem %d D %d H %d u %d", elem, D, H, u);
                        CHECK(gqa_kv_unit(u, lg, 1) == u, "g = 1 is the identity: elem %d D %d H %d u %d", elem, D, H, u);
                    }
                    // every K/V unit is loaded by exactly g lanes
                    for (int k = 0; k < Dkvu; ++k) {
                        int n = 0;
                        for (int u = 0; u < Du; ++u) n += gqa_kv_unit(u, lg, g) == k;
                        CHECK(n == g, "elem %d D %d H %d Hkv %d: K/V unit %d loaded by %d lanes", elem, D, H, Hkv, k, n);
                    }
                }
            }
        }
    }
    return shapes;
}

struct Shape {
    int B, S, D, H, Hkv, elem, ok;
};
const Shape kShapes[] = {
    // accepted: the shapes of tests/gqa_model.py and the measured ones
    {40, 64, 64, 2, 1, MLI_ELEM_F32, 1},
    {24, 256, 512, 8, 4, MLI_ELEM_F32, 1},
    {24, 256, 512, 8, 2, MLI_ELEM_BF16, 1},
    {24, 256, 512, 8, 1, MLI_ELEM_BF16, 1},
    {24, 256, 512, 8, 8, MLI_ELEM_F32, 1},      // no grouping is a grouping of one
    {24, 256, 192, 3, 1, MLI_ELEM_F32, 1},      // g = 3
    {24, 256, 192, 6, 2, MLI_ELEM_BF16, 1},     // g = 3, head_dim 32
    {24, 256, 192, 6, 3, MLI_ELEM_F32, 1},
    {24, 512, 1024, 8, 2, MLI_ELEM_BF16, 1},
    {1024, 4096, 512, 16, 4, MLI_ELEM_BF16, 1},
    {256, 1024, 256, 4, 1, MLI_ELEM_F32, 1},
    {16384, 64, 128, 2, 1, MLI_ELEM_F32, 1},
    // refused: the counts
    {24, 256, 512, 8, 3, MLI_ELEM_F32, 0},      // not a divisor
    {24, 256, 512, 8, 5, MLI_ELEM_BF16, 0},
    {24, 256, 512, 8, 16, MLI_ELEM_F32, 0},     // more K/V heads than heads
    {24, 256, 512, 8, 0, MLI_ELEM_F32, 0},
    {24, 256, 512, 8, -2, MLI_ELEM_F32, 0},
    {24, 256, 192, 6, 4, MLI_ELEM_F32, 0},
    // refused: one head (the single-head scan has no groups), and what the multi-head scan refuses
    {24, 256, 512, 1, 1, MLI_ELEM_F32, 0},
    {24, 256, 512, 0, 1, MLI_ELEM_F32, 0},
    {24, 256, 512, 8, 4, MLI_ELEM_FP8, 0},      // fp8 pages
    {24, 256, 512, 8, 4, 3, 0},                 // no such element type
    {8, 64, 128, 8, 4, MLI_ELEM_F32, 0},        // head_dim 16
    {8, 64, 1024, 2, 1, MLI_ELEM_BF16, 0},      // head_dim 512
    {8, 64, 128, 3, 1, MLI_ELEM_F32, 0},        // emb_dim % n_heads
    {8, 64, 1024, 8, 4, MLI_ELEM_F32, 0},       // fp32 rows wider than two lane loads
    {8, 64, 2048, 8, 4, MLI_ELEM_BF16, 0},      // bf16 rows wider than two lane loads
    {8, 72, 128, 2, 1, MLI_ELEM_F32, 0},        // n_sequence % 16
    {16385, 64, 128, 2, 1, MLI_ELEM_F32, 0},    // more rows than arrival counters
    {0, 64, 128, 2, 1, MLI_ELEM_F32, 0},
    {2, 131088, 1024, 32, 8, MLI_ELEM_BF16, 0},  // a row's (items x heads) statistics beyond the merge's LDS
};

void check_plan_field_by_field(const char* what, const ScanPlan& a, const ScanPlan& b, bool nt_too) {
    CHECK(a.ct == b.ct, "%s: ct %d / %d", what, a.ct, b.ct);
    CHECK(a.nchunk == b.nchunk, "%s: nchunk", what);
    CHECK(a.direct == b.direct, "%s: direct", what);
    CHECK(a.grid_y == b.grid_y, "%s: grid_y", what);
    CHECK(a.stats_bytes == b.stats_bytes, "%s: stats_bytes", what);
    CHECK(a.body_bytes == b.body_bytes, "%s: body_bytes", what);
    if (nt_too) CHECK(a.nt == b.nt, "%s: nt", what);
}

int check_plans() {
    int plans = 0;
    for (int chunk : {0, 64, 256, 1024})
        for (int order : {0, 1})
            for (int ntl : {0, 1, 2}) {
                const ScanTune t{chunk, order, ntl};
                for (int esize : {4, 2})
                    for (int B : {1, 20, 24, 256, 700, 1024, 2048})
                        for (int S : {64, 128, 1024, 4096})
                            for (int span : {S, window_span(S, 100), sink_span(S, 100, 20)})
                                for (int D : {64, 192, 256, 512})
                                    for (int H : {1, 2, 4, 8}) {
                                        if (D % H) continue;
                                        char what[128];
                                        std::snprintf(what, sizeof what, "tune (%d %d %d) e %d B %d S %d span %d D %d H %d", chunk,
                                                      order, ntl, esize, B, S, span, D, H);
                                        const ScanPlan old = plan_chunked_scan(t, B, S, span, D, H, esize);
                                        // read width D: today's plan
                                        check_plan_field_by_field(what, plan_chunked_scan(t, B, S, span, D, D, H, esize), old, true);
                                        // a narrower read width: the cache policy is judged by the bytes read, nothing else moves
                                        for (int Hkv = 1; Hkv < H; ++Hkv) {
                                            if (H % Hkv) continue;
                                            const int Dkv = D / H * Hkv;
                                            const ScanPlan p = plan_chunked_scan(t, B, S, span, D, Dkv, H, esize);
                                            check_plan_field_by_field(what, p, old, false);
                                            CHECK(p.nt == nt_loads_rule(ntl, B, span, Dkv, esize), "%s Hkv %d: nt", what, Hkv);
                                            CHECK(p.nt == plan_chunked_scan(t, B, S, span, Dkv, H, esize).nt, "%s Hkv %d: nt", what, Hkv);
                                        }
                                        ++plans;
                                    }
            }
    // the rule bites: 1024 rows x 4096 tokens x 512 bf16 columns are 8 GiB of K/V (non-temporal), a sixteenth of the
    // columns are 512 MiB (default policy: a good part can stay on die)
    const ScanTune t{0, 1, 2};
    CHECK(plan_chunked_scan(t, 1024, 4096, 4096, 512, 512, 16, 2).nt, "config 4, every column read");
    CHECK(plan_chunked_scan(t, 1024, 4096, 4096, 512, 128, 16, 2).nt, "config 4, a quarter of the columns: 2 GiB");
    CHECK(!plan_chunked_scan(t, 1024, 4096, 4096, 512, 32, 16, 2).nt, "config 4, one K/V head of 16: 512 MiB");
    return plans;
}

}  // namespace

int main() {
    const int shapes = check_lane_map();
    int rows = 0;
    for (const Shape& s : kShapes) {
        CHECK(gqa_shape_supported(s.B, s.S, s.D, s.H, s.Hkv, s.elem) == s.ok, "B %d S %d D %d H %d Hkv %d elem %d", s.B, s.S, s.D,
              s.H, s.Hkv, s.elem);
        // ... which is the windowed scan's answer for several heads, and the two conditions on the counts
        const bool want = s.H > 1 && window_shape_supported(s.B, s.S, s.D, s.H, s.elem) && s.Hkv >= 1 && s.Hkv <= s.H &&
                          s.H % (s.Hkv > 0 ? s.Hkv : 1) == 0;
        CHECK((gqa_shape_supported(s.B, s.S, s.D, s.H, s.Hkv, s.elem) != 0) == want, "B %d S %d D %d H %d Hkv %d elem %d: rule", s.B,
              s.S, s.D, s.H, s.Hkv, s.elem);
        ++rows;
    }
    const int plans = check_plans();
    std::printf("%d lane-map shapes, %d shape rows, %d plans, %d failure(s)\n", shapes, rows, plans, failures);
    return failures == 0 ? 0 : 1;
}
