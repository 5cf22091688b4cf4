// Longest-first row order of the one-workgroup-per-row grids of the chunked paged scans (when it applies: scan_plan.hpp).
#pragma once

#include "scan_item_body.hpp"
#include "scan_plan.hpp"

namespace mli {

// One workgroup per row (short sequences: the whole row is one item): workgroups start in grid order and the rows' lengths
// are ragged, so whichever long rows happen to sit at the end of the grid run alone at the end (README workload, B=1024,
// S=128, D=2048: 5.3 TB/s against 6.4 with equal lengths).  This hands the rows out LONGEST FIRST instead: workgroup r takes
// the row of rank r by page count (descending; equal counts in row order).  Every workgroup derives the same ranking from
// the lengths -- a histogram over the page counts, then the j-th row of its bucket by a block-wide count --: ~2 us of
// prologue per workgroup, no pre-pass, deterministic.  All kFuThreads threads call it; n_batch <= kMaxOrderedRows.
// WIN = true (the windowed scans): the rows are ranked by the pages their window leaves live, ceil(L / 16) - lo / 16 with
// lo = max(0, L - window); S / 16 may then exceed kMaxOrderedPages as long as the window's span does not.
// SINK = true (with WIN): ... by the pages of the virtual row, ceil(L / 16) - max(0, lo / 16 - ceil(n_sink / 16)).
template <bool WIN = false, bool SINK = false>
__device__ __forceinline__ int longest_first_row(const int* __restrict__ lengths, int n_batch, int S, int rank, int window = 0,
                                                 int n_sink = 0) {
    __shared__ int hist[kMaxOrderedPages + 1];
    __shared__ int wave_cnt[kFuWaves];
    __shared__ int found_row;
    constexpr int kPer = kMaxOrderedRows / kFuThreads;
    const int tid = threadIdx.x;
    const int per = (n_batch + kFuThreads - 1) / kFuThreads;  // rows per thread, a contiguous segment
    if (tid <= kMaxOrderedPages) hist[tid] = 0;
    __syncthreads();
    int pages[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int row = tid * per + j;
        pages[j] = -1;
        if (j < per && row < n_batch) {
            const int len = min(max(lengths[row], 0), S);
            // (the old expression stays verbatim in the else branch: with the pages below the window as a named value the
            // windowed kernels' instruction order changes)
            if constexpr (SINK)
                pages[j] = (len + kPage - 1) / kPage - max(0, max(0, len - window) / kPage - (n_sink + kPage - 1) / kPage);
            else
                pages[j] = (len + kPage - 1) / kPage - (WIN ? max(0, len - window) / kPage : 0);
            atomicAdd(&hist[pages[j]], 1);
        }
    }
    __syncthreads();
    // the bucket of this rank (page counts descending) and the rank inside it
    int bucket = 0, before = 0;
    for (int p = kMaxOrderedPages; p >= 0; --p) {
        const int h = hist[p];
        if (rank < before + h) {
            bucket = p;
            break;
        }
        before += h;
    }
    const int j_in_bucket = rank - before;
    // the j-th row of the bucket in row order: matches per thread segment, exclusive prefix over the threads
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) mine += pages[j] == bucket;
    int incl = mine;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int up = __shfl_up(incl, off, kWave);
        if ((tid & (kWave - 1)) >= off) incl += up;
    }
    if ((tid & (kWave - 1)) == kWave - 1) wave_cnt[tid / kWave] = incl;
    __syncthreads();
    int base = incl - mine;
    for (int w = 0; w < tid / kWave; ++w) base += wave_cnt[w];
    if (j_in_bucket >= base && j_in_bucket < base + mine) {
        int seen = base;
#pragma unroll
        for (int j = 0; j < kPer; ++j) {
            if (pages[j] == bucket) {
                if (seen == j_in_bucket) found_row = tid * per + j;
                ++seen;
            }
        }
    }
    __syncthreads();
    return found_row;
}

}  // namespace mli
