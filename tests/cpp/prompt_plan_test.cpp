// Prompt log-probabilities on the host side (min_llm_inference_amd/csrc/prompt_plan.hpp, scan_plan.hpp), CPU only: both headers
// are plain C++ and are compiled here without HIP.
//   - cut_prompt_passes: no pass exceeds the limit, every position 0 .. L - 2 of every row appears exactly once and in order,
//     the offsets of a pass tile [0, n_positions), a continuation has first > 0; prompts of length 1, 2, limit, limit + 1 and
//     n_sequence, alone and mixed;
//   - prompt_scan_shape_ok against a table of accepted and refused shapes, and prompt_scan_tq >= 2 for every variant.
#include <cstdio>
#include <initializer_list>
#include <utility>
#include <vector>

#include "prompt_plan.hpp"
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

void check_passes(const std::vector<PromptRow>& rows, int limit, const char* what) {
    const std::vector<PromptPass> passes = cut_prompt_passes(rows, limit);
    std::vector<std::pair<int, int>> got, want;   // (row, position) in the order scored / in the order due
    for (const PromptRow& r : rows)
        for (int t = 0; t + 1 < r.n_prompt; ++t) want.emplace_back(r.row, t);
    for (size_t i = 0; i < passes.size(); ++i) {
        const PromptPass& p = passes[i];
        CHECK(p.n_positions >= 1 && p.n_positions <= limit, "%s: pass %zu has %d positions, limit %d", what, i, p.n_positions, limit);
        CHECK(i + 1 == passes.size() || p.n_positions == limit, "%s: pass %zu is not full but not the last", what, i);
        int at = 0, longest = 0;
        for (const PromptSegment& g : p.segments) {
            CHECK(g.count >= 1 && g.first >= 0, "%s: empty segment", what);
            CHECK(g.offset == at, "%s: offsets do not tile the pass", what);
            for (int t = 0; t < g.count; ++t) got.emplace_back(g.row, g.first + t);
            at += g.count;
            if (g.count > longest) longest = g.count;
        }
        CHECK(at == p.n_positions && longest == p.max_count, "%s: pass %zu counts", what, i);
    }
    CHECK(got == want, "%s: %zu positions scored, %zu due, or not in order", what, got.size(), want.size());
}

}  // namespace

int main() {
    const int n_batch = 8, n_sequence = 128;
    for (int L : {1, 2, n_batch, n_batch + 1, n_sequence, n_sequence - 1, 3, 17})
        check_passes({PromptRow{0, L}}, n_batch, "one row");
    check_passes({{3, 1}, {0, 2}, {5, n_batch}, {1, n_batch + 1}, {7, n_sequence}, {2, 1}, {4, 9}}, n_batch, "mixed rows");
    check_passes({{0, n_sequence}, {1, n_sequence}, {2, n_sequence}}, n_batch, "long rows");
    check_passes({{0, 2}, {1, 2}, {2, 2}, {3, 2}, {4, 2}, {5, 2}, {6, 2}, {7, 2}}, n_batch, "eight rows of one position");
    check_passes({{6, 5}, {2, 5}}, 1, "a limit of one");
    check_passes({{6, 5}, {2, 5}}, 1000, "a limit beyond everything");
    CHECK(cut_prompt_passes({{0, 1}, {1, 0}, {2, -4}}, n_batch).empty(), "rows with nothing to score");
    CHECK(cut_prompt_passes({{0, 9}}, 0).empty() && cut_prompt_passes({{0, 9}}, -1).empty(), "no limit, no passes");
    {   // a prompt of n_batch + 1 tokens is one full pass; one more token spills a single position into a second pass
        const auto a = cut_prompt_passes({{0, n_batch + 1}}, n_batch), b = cut_prompt_passes({{0, n_batch + 2}}, n_batch);
        CHECK(a.size() == 1 && a[0].n_positions == n_batch, "n_batch positions");
        CHECK(b.size() == 2 && b[1].segments.size() == 1 && b[1].segments[0].first == n_batch && b[1].segments[0].count == 1,
              "the continuation");
    }

    struct Shape { int B, S, D, H, Hkv, elem; bool ok; };
    const Shape table[] = {
        {8, 128, 64, 1, 1, MLI_ELEM_F32, true},    {8, 128, 512, 1, 1, MLI_ELEM_F32, true},    {8, 128, 516, 1, 1, MLI_ELEM_F32, false},
        {8, 128, 1024, 1, 1, MLI_ELEM_BF16, true}, {8, 128, 1032, 1, 1, MLI_ELEM_BF16, false}, {8, 128, 1024, 1, 1, MLI_ELEM_F32, false},
        {8, 128, 66, 1, 1, MLI_ELEM_F32, false},   {8, 120, 128, 1, 1, MLI_ELEM_F32, false},   {0, 128, 128, 1, 1, MLI_ELEM_F32, false},
        {16384, 128, 128, 1, 1, MLI_ELEM_F32, true}, {16385, 128, 128, 1, 1, MLI_ELEM_F32, false},
        {8, 128, 128, 4, 4, MLI_ELEM_F32, true},   {8, 128, 64, 4, 4, MLI_ELEM_F32, false},    {8, 128, 1024, 8, 2, MLI_ELEM_BF16, true},
        {8, 128, 256, 8, 1, MLI_ELEM_F32, true},   {8, 128, 256, 8, 3, MLI_ELEM_F32, false},   {8, 128, 256, 8, 16, MLI_ELEM_F32, false},
        {8, 128, 256, 1, 2, MLI_ELEM_F32, false},  {8, 128, 256, 0, 1, MLI_ELEM_F32, false},   {8, 128, 256, 8, 0, MLI_ELEM_F32, false},
        {8, 128, 256, 1, 1, MLI_ELEM_FP8, false},  {8, 128, 256, 4, 4, MLI_ELEM_FP8, false},   {8, 128, 256, 1, 1, 3, false},
    };
    for (const Shape& s : table)
        CHECK(prompt_scan_shape_ok(s.B, s.S, s.D, s.H, s.Hkv, s.elem) == s.ok, "shape B %d S %d D %d H %d Hkv %d elem %d", s.B, s.S,
              s.D, s.H, s.Hkv, s.elem);
    for (int epl : {4, 8})
        for (int nj : {1, 2})
            for (bool heads : {false, true}) {
                const int tq = prompt_scan_tq(epl, nj, heads);
                CHECK(tq == 2 || tq == 4 || tq == 8, "TQ %d for epl %d nj %d heads %d", tq, epl, nj, (int)heads);
            }
    // the grid: fewer than 2^32 work items in x, that is at most 2^24 - 1 workgroups of 256 threads
    for (int tq : {2, 4, 8}) {
        const int nb = (4096 + tq - 1) / tq;
        const int last = ((1 << 24) - 1) / nb;   // the most segments of max_count 4096
        CHECK(prompt_scan_grid_ok(last, 4096, tq) && !prompt_scan_grid_ok(last + 1, 4096, tq), "grid at TQ %d: %d segments", tq, last);
    }
    CHECK(prompt_scan_grid_ok((1 << 24) - 1, 1, 8) && !prompt_scan_grid_ok(1 << 24, 1, 8), "grid with one block per segment");
    CHECK(prompt_scan_grid_ok(0x7fffffff / 4096, 1, 8) && !prompt_scan_grid_ok(0x7fffffff, 4096, 2), "no overflow in the product");
    if (failures == 0) std::printf("prompt_plan_test: all checks passed\n");
    return failures == 0 ? 0 : 1;
}
