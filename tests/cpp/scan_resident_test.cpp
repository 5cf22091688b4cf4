// The resident slice of the equal-shares scan (min_llm_inference_amd/csrc/scan_plan.hpp: resident_threshold and
// resident_keeps -- the text the kernel compiles), CPU only: the threshold at its edges and at the largest shape the kernel
// takes, monotonicity of the keep rule in the threshold, and the share of pages it keeps on page pools laid out as the
// engines and the benchmark lay them out (base + block * permutation).
#include <cstdint>
#include <cstdio>
#include <cmath>
#include <numeric>
#include <vector>

#include "scan_plan.hpp"

using namespace mli;

namespace {

int failures = 0;

#define CHECK(cond, ...)                          \
    do {                                          \
        if (!(cond)) {                            \
            std::printf("[FAIL] " __VA_ARGS__);   \
            std::printf("\n");                    \
            ++failures;                           \
        }                                         \
    } while (0)

static_assert(resident_threshold(1000, 32768, 0) == 0u, "usable in constant expressions");

void test_threshold() {
    const long long kv = 2LL * 16 * 512 * 2;   // bf16, D = 512
    CHECK(resident_threshold(130000, kv, 0) == 0u, "0 MiB keeps nothing");
    CHECK(resident_threshold(130000, kv, -5) == 0u, "a negative size keeps nothing");
    CHECK(resident_threshold(0, kv, 192) == 65536u, "no pages: everything (of nothing)");
    CHECK(resident_threshold(0, kv, 0) == 0u, "0 MiB wins over no pages");
    CHECK(resident_threshold(1, kv, 1) == 65536u, "one page of 32 KiB under 1 MiB: all, clamped");
    CHECK(resident_threshold(100, kv, 240) == 65536u, "3.2 MB under 240 MiB: all, clamped");
    // 192 MiB of 129000 pages of 32 KiB: 192 * 2^20 * 2^16 / (129000 * 2^15) = 402653184 / 129000 = 3121.3
    CHECK(resident_threshold(129000, kv, 192) == 3121u, "config 4, bf16: got %u", resident_threshold(129000, kv, 192));
    // 8192 pages of 32 KiB are 256 MiB: 192 MiB are exactly three quarters
    CHECK(resident_threshold(8192, kv, 192) == 49152u, "three quarters: got %u", resident_threshold(8192, kv, 192));
    // the largest shape: 2048 rows x 256 pages x 64 KiB = 2^35 bytes; 240 MiB of it are 240 * 2^36 / 2^35 = 480 of 65536.
    // (in 32-bit arithmetic the byte count is 0 and the product 240 << 36 as well)
    CHECK(resident_threshold(2048LL * 256, 65536, 240) == 480u, "largest shape: got %u", resident_threshold(2048LL * 256, 65536, 240));
    CHECK(resident_threshold(2048LL * 256, 65536, 1) == 2u, "largest shape, 1 MiB: got %u", resident_threshold(2048LL * 256, 65536, 1));
    unsigned prev = 0;
    for (int mib = 0; mib <= 240; ++mib) {   // monotone in the size
        const unsigned t = resident_threshold(129000, kv, mib);
        CHECK(t >= prev && t <= 65536u, "threshold not monotone at %d MiB", mib);
        prev = t;
    }
}

std::vector<uint64_t> page_pool(uint64_t base, uint64_t block, int n, uint64_t seed) {
    std::vector<uint32_t> perm(n);
    std::iota(perm.begin(), perm.end(), 0u);
    for (int i = n - 1; i > 0; --i) {   // Fisher-Yates with xorshift
        seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
        const int j = (int)(seed % (uint64_t)(i + 1));
        const uint32_t t = perm[i]; perm[i] = perm[j]; perm[j] = t;
    }
    std::vector<uint64_t> p(n);
    for (int i = 0; i < n; ++i) p[i] = base + block * perm[i];
    return p;
}

const int kDE[][2] = {{64, 4}, {64, 2}, {64, 1}, {512, 4}, {512, 2}, {512, 1}, {1024, 2}, {1024, 1}};
const uint64_t kBases[] = {0x7f3a00000000ull, 0x7e0012345100ull, 0x7fc4d2e01300ull};
const int kPages = 60000;

void test_monotone() {
    const unsigned thr[] = {0, 1, 2, 100, 3014, 3015, 21845, 32768, 43690, 65535, 65536};
    const std::vector<uint64_t> pool = page_pool(kBases[1], 16 * 3 * 512 * 2, kPages, 88172645463325252ull);
    long long bad = 0, kept0 = 0, dropped_all = 0;
    for (uint64_t p : pool) {
        bool before = false;
        for (unsigned t : thr) {
            const bool k = resident_keeps(p, t);
            if (before && !k) ++bad;   // a page kept under a threshold is kept under every larger one
            before = k;
        }
        kept0 += resident_keeps(p, 0);
        dropped_all += !resident_keeps(p, 65536);
    }
    CHECK(bad == 0, "%lld pages leave the slice as the threshold grows", bad);
    CHECK(kept0 == 0, "threshold 0 keeps %lld pages", kept0);
    CHECK(dropped_all == 0, "threshold 65536 drops %lld pages", dropped_all);
}

void test_fraction() {
    const double fractions[] = {0.01, 0.046, 0.1, 1.0 / 3, 0.5, 2.0 / 3, 0.9};
    int sets = 0;
    for (const auto& de : kDE)
        for (uint64_t base : kBases) {
            const uint64_t block = 16ull * 3 * de[0] * de[1];
            const std::vector<uint64_t> pool = page_pool(base, block, kPages, 88172645463325252ull + block);
            ++sets;
            for (double f : fractions) {
                const unsigned thr = (unsigned)(f * 65536);
                long long kept = 0;
                for (uint64_t p : pool) kept += resident_keeps(p, thr);
                const double want = thr / 65536.0, got = (double)kept / kPages;
                CHECK(std::fabs(got - want) <= 0.02 * want, "D %d e %d base %llx: kept %.5f of the pages, threshold says %.5f",
                      de[0], de[1], (unsigned long long)base, got, want);
            }
            // shares of 256 consecutive pages of the shuffled sequence, as a workgroup's share at config 4: at 4.6 % the
            // mean count per share is what the threshold says
            const unsigned thr = (unsigned)(0.046 * 65536);
            const int shares = kPages / 256;
            long long kept = 0;
            int lo = 256, hi = 0;
            for (int s = 0; s < shares; ++s) {
                int c = 0;
                for (int i = 0; i < 256; ++i) c += resident_keeps(pool[(size_t)s * 256 + i], thr);
                kept += c;
                lo = c < lo ? c : lo;
                hi = c > hi ? c : hi;
            }
            const double mean = (double)kept / shares, want = 256.0 * thr / 65536.0;
            CHECK(std::fabs(mean - want) <= 0.02 * want, "D %d e %d base %llx: %.3f pages per share of 256, expected %.3f (%d .. %d)",
                  de[0], de[1], (unsigned long long)base, mean, want, lo, hi);
        }
    std::printf("%d page pools of %d pages\n", sets, kPages);
}

}  // namespace

int main() {
    test_threshold();
    test_monotone();
    test_fraction();
    std::printf("scan_resident_test: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
