// Prompt log-probabilities (attention_prompt.hpp): how the host cuts the prompts of a forward's new rows into passes of at most
// `limit` query positions, so that the materialised logits of a pass fit [limit, n_vocab].  Plain C++ over ints and vectors, no
// HIP types and no global state (tests/cpp/prompt_plan_test.cpp compiles it alone, beside scan_plan.hpp's shape predicate).
#pragma once

#include <vector>

namespace mli {

struct PromptRow {
    int row;        // batch row
    int n_prompt;   // tokens the row's item was queued with: positions 0 .. n_prompt - 2 are scored (position i for token i + 1)
};
struct PromptSegment {
    int row, first, count, offset;   // positions first .. first + count - 1 of `row`, at rows offset .. of the pass's dense arrays
};
struct PromptPass {
    std::vector<PromptSegment> segments;
    int n_positions = 0;   // <= limit: the segments' offsets tile [0, n_positions)
    int max_count = 0;
};

// Rows in the order given, positions in order; a row that does not fit the rest of a pass continues in the next one as a
// segment with first > 0.  A row of fewer than two tokens has nothing to score.  limit < 1: no passes.
inline std::vector<PromptPass> cut_prompt_passes(const std::vector<PromptRow>& rows, int limit) {
    std::vector<PromptPass> passes;
    if (limit < 1) return passes;
    for (const PromptRow& r : rows) {
        int first = 0;
        int left = r.n_prompt - 1;
        while (left > 0) {
            if (passes.empty() || passes.back().n_positions == limit) passes.emplace_back();
            PromptPass& p = passes.back();
            const int room = limit - p.n_positions;
            const int count = left < room ? left : room;
            p.segments.push_back(PromptSegment{r.row, first, count, p.n_positions});
            p.n_positions += count;
            if (count > p.max_count) p.max_count = count;
            first += count;
            left -= count;
        }
    }
    return passes;
}

}  // namespace mli
