// CPU test of early page release (csrc/page_live.hpp and PagedAttentionsManager::set_page_release), stand-alone under ASan
// + UBSan over the malloc test double.
//   1. The rule, against an independent restatement from the scan's slot mask: page i is READ at length L iff some slot s
//      of it has s < L and (s < K or s >= L - W).
//   2. The scheduler, with a FAKE windowed model over real pages: prefill and every decode round write the owning (item id,
//      position) into the slots they fill, and every forward checks that each slot it reads lies on a page that is there
//      and carries its own row's tag -- a page released too early and handed to another row does not.  Sequential and
//      pipelined loop, roomy to tiny pools, against the release-off run of the same loop in a roomy pool.
// Built with -DMUTANT=k (a deliberate fault in paged_item_storage.cpp, 1 .. 6) the program must FAIL: the test that builds
// it (tests/test_page_release_cpu.py) checks that too.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <map>
#include <random>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../min_llm_inference_amd/csrc/page_live.hpp"
#include "constants.h"
#include "pipelined_engine.h"
#include "throughput_counter.h"

static int g_failures = 0;
#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            if (g_failures < 20) std::printf("  CHECK failed: %s  (%s:%d)\n", #cond, __FILE__, __LINE__); \
            ++g_failures;                                                           \
        }                                                                           \
    } while (0)

constexpr int P = PAGE_BLOCK_SIZE;

// ---- 1. the rule ---------------------------------------------------------------------------------------------------
// bit i of the result: page i is read by the scan of a row of L tokens (the slot mask of scan_item_body.hpp, restated)
static uint32_t pages_read(int L, int W, int K) {
    uint32_t m = 0;
    for (int s = 0; s < L; ++s)
        if (s < K || s >= L - W) m |= 1u << (s / P);
    return m;
}

static void rule_cases(int S) {
    const int width = S / P;
    long long cases = 0, attained = 0, attainable = 0;
    std::vector<uint32_t> read(S + 1), later(S + 2);
    for (int W = 1; W < S; ++W)
        for (int K = 0; K + W < S; ++K) {
            later[S + 1] = 0;
            for (int L = S; L >= 0; --L) {
                read[L] = pages_read(L, W, K);
                later[L] = later[L + 1] | read[L];   // read at some L' >= L
            }
            int most[3] = {0, 0, 0};
            const int aheads[3] = {1, 6, 16};
            for (int n = 0; n <= S; ++n) {
                uint32_t dead = 0;
                for (int i = 0; i < width; ++i)
                    if (mli::page_dead(i, n, W, K)) dead |= 1u << i;
                CHECK((dead & later[n]) == 0);          // dead at n: read at no L >= n
                CHECK((read[n] & ~dead) == read[n]);    // live at n: every page read at n
                // the live tokens: in order, onto exactly the tokens of the pages that are not dead
                const int live = mli::live_tokens(n, W, K);
                int expect = 0, prev = -1, bad = 0;
                for (int i = 0; i * P < n; ++i) expect += (dead >> i & 1) ? 0 : std::min(P, n - i * P);   // tokens of live pages
                for (int j = 0; j < live; ++j) {
                    const int s = mli::live_slot(j, n, W, K);
                    bad += !(s > prev && s < n && !(dead >> (s / P) & 1));
                    prev = s;
                }
                CHECK(live == expect && bad == 0);
                CHECK(live <= mli::live_tokens_bound(S, W, K));
                for (int a = 0; a < 3; ++a) {
                    const int top = std::min(width, (n + aheads[a] + P - 1) / P);
                    int count = 0;
                    for (int i = 0; i < top; ++i) count += !(dead >> i & 1);
                    CHECK(mli::live_pages_covering(n, aheads[a], W, K, width) == count);
                    CHECK(count <= mli::live_pages_bound(aheads[a], W, K));
                    most[a] = std::max(most[a], count);
                }
                ++cases;
            }
            // attained wherever the row has room for it: a gap (n = W + 16 (ps + 1) + r), the look-ahead inside the row, and a
            // remainder r <= 15 that pushes window + look-ahead onto one more page ((W + a) % 16 != 1)
            for (int a = 0; a < 3; ++a) {
                const int bound = mli::live_pages_bound(aheads[a], W, K);
                if ((W + aheads[a]) % P != 1 && W + P * (mli::live_sink_pages(K) + 2) + aheads[a] <= S) {
                    ++attainable;
                    CHECK(most[a] == bound);
                }
                attained += most[a] == bound;
            }
        }
    CHECK(attainable > 0 && attained >= attainable);
    std::printf("%s the rule at S = %d: %lld (W, K, n), bound attained for %lld (W, K, look-ahead)\n",
                g_failures == 0 ? "[ OK ]" : "[FAIL]", S, cases, attained);
}

// ---- 2. the scheduler ----------------------------------------------------------------------------------------------
struct World {
    ItemStorage items;
    ProcessingStorage processing;
    MemoryBlockManager pool;
    PagedAttentionsManager pages;
    int n_blocks;
    // a page = 16 slots of (item id, position)
    World(size_t B, size_t S, int blocks) : pool(blocks, P * 2), pages(B, S, 4), n_blocks(blocks) {
        float** t = pages.get_page_table_device().data();   // the double hands out uninitialised memory
        for (size_t i = 0; i < B * (S / P); ++i) t[i] = nullptr;
    }
};

struct FakeModel {
    int B, S, W, K, eof_bias, rounds;
    World* w;
    std::vector<uint64_t> h;          // running hash per slot: the token is a function of the row's whole prefix
    std::vector<float> poison;        // what the dead entries of a new row are pointed at before its prefill
    long long launches = 0, faults = 0, shared_pages = 0;

    FakeModel(int B_, int S_, int W_, int K_, int eof, int R, World* world)
        : B(B_), S(S_), W(W_), K(K_), eof_bias(eof), rounds(R), w(world), h(B_, 0), poison(P * 2, -7.f) {}

    static uint64_t mix(uint64_t h, uint64_t x) {
        h ^= x + 0x9e3779b97f4a7c15ull + (h << 6) + (h >> 2);
        return h * 0xff51afd7ed558ccdull;
    }
    int token_of(uint64_t hh) const {
        if (static_cast<int>((hh >> 17) % 1000) < eof_bias) return EOF_TOKEN_ID;   // eof_bias in permille
        return static_cast<int>((hh >> 33) % EOF_TOKEN_ID);
    }
    bool attends(int s, int L) const { return s < L && (W <= 0 || s < K || s >= L - W); }
    // page i (holding tokens of a row of L) is read by some scan of the row from now on
    bool read_later(int i, int L) const {
        for (int n = L; n <= S; ++n)
            for (int s = i * P; s < (i + 1) * P; ++s)
                if (attends(s, n)) return true;
        return false;
    }
    float* slot(int b, int s) {
        float* page = w->pages.get_page_table_device().data()[b * (S / P) + s / P];
        if (page == nullptr || page == poison.data()) {
            ++faults;
            return nullptr;
        }
        return page + (s % P) * 2;
    }
    void write(int b, int id, int s) {
        if (float* t = slot(b, s)) { t[0] = static_cast<float>(id); t[1] = static_cast<float>(s); }
    }
    void read(int b, int id, int s) {
        if (float* t = slot(b, s)) faults += !(t[0] == static_cast<float>(id) && t[1] == static_cast<float>(s));
    }

    void forward(const TensorInt& inp, TensorInt& lengths, const TensorInt& new_idx, TensorInt& result, int n_new) {
        ++launches;
        const int* in = inp.data();
        int* len = lengths.data();
        int* res = result.data();
        float** table = w->pages.get_page_table_device().data();
        {   // no two rows hold the same page
            std::set<float*> held;
            for (const BatchIdMemoryBlocksPair& row : w->pages.get_used_block_list())
                for (float* page : row.second) shared_pages += !held.insert(page).second;
        }
        for (int i = 0; i < n_new; ++i) {   // prefill: the live tokens only, and no dead entry is followed
            const int b = new_idx.data()[i], L = len[b], id = w->processing.get_token(b).first;
            uint64_t hh = 0x1234;
            for (int s = 0; s < L; ++s) hh = mix(hh, static_cast<uint64_t>(in[b * S + s]));
            h[b] = hh;
            const bool windowed = w->pages.page_release();
            for (int p = 0; p * P < L; ++p) {
                if (windowed && !read_later(p, L)) {
                    table[b * (S / P) + p] = poison.data();
                    continue;
                }
                for (int s = p * P; s < std::min(L, (p + 1) * P); ++s) write(b, id, s);
            }
        }
        for (int r = 0; r < rounds; ++r)
            for (int b = 0; b < B; ++b) {
                const int L = len[b];
                if (L <= 0) {
                    res[b * rounds + r] = EMPTY_ROW_TOKEN_ID;
                    continue;
                }
                const int id = w->processing.get_token(b).first;
                // projection of the last token and the scan: the slots s with attends(s, L)
                const int sinks = std::min(W <= 0 ? L : K, L);
                for (int s = 0; s < sinks; ++s) read(b, id, s);
                for (int s = std::max(sinks, L - W); s < L; ++s) read(b, id, s);
                const int tok = token_of(h[b]);
                res[b * rounds + r] = tok;
                h[b] = mix(h[b], static_cast<uint64_t>(tok));
                if (L < S) write(b, id, L);         // the decoder appends the next embedding
                len[b] = (tok == EOF_TOKEN_ID || L + 1 >= S) ? 0 : L + 1;
            }
        for (float v : poison) faults += v != -7.f;
    }
};

static std::map<int, std::vector<int>> collect(const ItemStorage& s) {
    std::map<int, std::vector<int>> out;
    for (const auto& it : s.get_finished_items()) out[it.first] = it.second;
    return out;
}

// the reference's loop order from the scheduler primitives; -1 = the pool is too small for the next queued item
static long long run_sequential(World& w, FakeModel& model, size_t B, size_t S, int R) {
    TensorInt inp_d({B, S}, DeviceType::DEVICE), inp_h({B, S}, DeviceType::HOST);
    TensorInt len_d({B}, DeviceType::DEVICE), len_h({B}, DeviceType::HOST);
    TensorInt idx_d({B}, DeviceType::DEVICE), idx_h({B}, DeviceType::HOST);
    TensorInt res_d({B, (size_t)R}, DeviceType::DEVICE), res_h({B, (size_t)R}, DeviceType::HOST);
    for (size_t b = 0; b < B; ++b) len_h.data()[b] = len_d.data()[b] = 0;
    std::vector<int> fresh = insert_new_items(inp_d, inp_h, len_d, len_h, idx_d, idx_h, w.items, w.processing, w.pool, w.pages, R);
    if (w.processing.size() == 0 && w.items.new_count() > 0) return -1;
    long long steps = 0;
    while (!is_done(w.items, w.processing)) {
        model.forward(inp_d, len_d, idx_d, res_d, static_cast<int>(fresh.size()));
        std::vector<int> finished = process_decoder_result(res_d, res_h, w.items, w.processing, static_cast<int>(S));
        allocate_or_free_memory_blocks_if_needed(w.pages, w.pool, w.processing, w.items, finished, R);
        fresh = insert_new_items(inp_d, inp_h, len_d, len_h, idx_d, idx_h, w.items, w.processing, w.pool, w.pages, R);
        if (w.processing.size() == 0 && w.items.new_count() > 0) return -1;
        if (++steps > 200000) return -2;
    }
    return steps;
}

struct Outcome {
    bool finished = false;       // false: the pool was reported as too small
    std::map<int, std::vector<int>> tokens;
    long long faults = 0, shared = 0, released = 0, preemptions = 0;
    int peak = 0;
    bool pool_whole = false;
};

static Outcome run(const std::vector<IdTokensPair>& items, bool pipelined, bool release, int B, int S, int W, int K, int R,
                   int n_blocks, int eof_bias) {
    World w(B, S, n_blocks);
    if (release) w.pages.set_page_release(W, K);
    for (const auto& it : items) w.items.add_new_item(IdTokensPair(it));
    FakeModel model(B, S, W, K, eof_bias, R, &w);
    get_global_throughput_counter().reset();
    get_global_throughput_counter().start_record();
    Outcome o;
    if (pipelined) {
        try {
            run_paged_engine_pipelined(w.items, w.processing, w.pool, w.pages, B, S,
                                       [&](const TensorInt& inp, TensorInt& len, const TensorInt& idx, TensorInt& res, int n_new) {
                                           if (model.launches > 200000) throw std::logic_error("no progress");
                                           model.forward(inp, len, idx, res, n_new);
                                       }, R);
            o.finished = true;
        } catch (const std::runtime_error&) {
        }
    } else {
        o.finished = run_sequential(w, model, B, S, R) >= 0;
    }
    o.tokens = collect(w.items);
    o.faults = model.faults;
    o.shared = model.shared_pages;
    o.released = w.pages.pages_released_early();
    o.preemptions = w.pages.preemptions();
    o.peak = w.pool.peak_pages_in_use();
    if (o.finished) {   // at the end the pool holds every page exactly once
        o.pool_whole = w.pool.free_blocks_size() == n_blocks && w.pages.get_used_block_list().empty();
        if (o.pool_whole) {
            std::list<float*> all = w.pool.pop_free_blocks(n_blocks);
            o.pool_whole = std::set<float*>(all.begin(), all.end()).size() == static_cast<size_t>(n_blocks);
            w.pool.return_free_blocks(std::move(all));
        }
    }
    return o;
}

static void scheduler_cases() {
    const int B = 8, S = 256, n_items = 40;
    std::mt19937 rng(4242);
    std::vector<IdTokensPair> items;
    for (int i = 0; i < n_items; ++i) {
        const int n = i < 6 ? std::vector<int>{1, 16, 200, 64, 17, 128}[i] : 1 + static_cast<int>(rng() % 200);   // 1 .. 200
        std::vector<int> toks(n);
        for (int& t : toks) t = static_cast<int>(rng() % EOF_TOKEN_ID);
        items.emplace_back(i, toks);
    }
    const int windows[4][2] = {{12, 0}, {12, 4}, {40, 20}, {17, 16}};
    int runs = 0;
    for (int pipelined = 0; pipelined < 2; ++pipelined)
        for (int R : {1, 3, 8})
            for (const auto& wk : windows) {
                const int W = wk[0], K = wk[1];
                const int before = g_failures;
                const int ahead = pipelined ? 2 * R : R;
                const int bound = mli::live_pages_bound(ahead, W, K);
                for (int eof : {4, 0}) {   // rows that end on EOF somewhere (0.4 % per token), and rows that all run to S
                    // the release-off run of the same loop in a roomy pool: what every run below must reproduce
                    const Outcome ref = run(items, pipelined, false, B, S, W, K, R, B * S / P, eof);
                    CHECK(ref.finished && (int)ref.tokens.size() == n_items && ref.faults == 0 && ref.released == 0);
                    CHECK(ref.pool_whole && ref.preemptions == 0);
                    const int pools[4] = {B * S / P, B * bound, bound + 2, S / P - 1};
                    for (int k = 0; k < 4; ++k) {
                        const Outcome o = run(items, pipelined, true, B, S, W, K, R, pools[k], eof);
                        CHECK(o.finished);
                        CHECK(o.tokens == ref.tokens);
                        CHECK(o.faults == 0 && o.shared == 0);
                        CHECK(o.pool_whole);
                        CHECK(o.released > 0);
                        CHECK(o.peak <= B * bound && o.peak <= pools[k]);
                        if (k <= 1) CHECK(o.preemptions == 0);
                        if (k == 2 && eof == 0) CHECK(o.preemptions > 0);   // 8 slots, pages for one long row and a bit
                        ++runs;
                    }
                    if (eof == 0) {   // every row needs S / 16 pages in the end: without release the pool is too small
                        const Outcome off = run(items, pipelined, false, B, S, W, K, R, S / P - 1, eof);
                        CHECK(!off.finished && off.faults == 0);
                        ++runs;
                    }
                }
                std::printf("%s %s loop, R = %d, W = %d, K = %d: per-row bound %d pages\n", g_failures == before ? "[ OK ]" : "[FAIL]",
                            pipelined ? "pipelined" : "sequential", R, W, K, bound);
            }
    std::printf("%d scheduler runs\n", runs);
}

// no argument: everything; "rule" / "scheduler": that part alone (the mutants differ in the scheduler only)
int main(int argc, char** argv) {
    const std::string part = argc > 1 ? argv[1] : "";
    if (part != "scheduler") {
        rule_cases(64);
        rule_cases(256);
    }
    if (part != "rule") scheduler_cases();
    std::printf("%d failure(s)\n", g_failures);
    return g_failures != 0;
}
