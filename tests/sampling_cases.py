"""Inputs and the comparison of the sampled-head tests, shared by tests/test_sampling_gpu.py and
tests/test_scratch_contract_gpu.py: logits with mixed per-row parameters, and a head's tokens held to the numpy reference
(sampling_ref) wherever its decision is well posed.

TEST INFRASTRUCTURE: never used by the product."""
import numpy as np

import sampling_ref as ref


def drawn_case(rng, B, V):
    """Logits with a spread that makes the draw non-degenerate, mixed T / K / P per row, ties at t_k, NaN / -inf / +inf
    entries, empty rows, and the out-of-domain parameter values the kernel must absorb."""
    x = (rng.standard_normal((B, V)) * rng.uniform(0.5, 2.0, (B, 1))).astype(np.float32)
    for b in range(B):               # a head of probable tokens over a long tail, as language-model logits have
        x[b, rng.choice(V, min(V, 48), replace=False)] += rng.uniform(4.0, 12.0, min(V, 48)).astype(np.float32)
    T = rng.choice(np.array([0.0, 0.3, 0.5, 0.7, 1.0], np.float32), B)
    K = rng.choice(np.array([0, 0, 1, 2, 5, 50, 400], np.int32), B)
    P = rng.choice(np.array([1.0, 1.0, 0.5, 0.9, 0.95, 0.2], np.float32), B)
    seed = rng.integers(-2 ** 63, 2 ** 63 - 1, B, dtype=np.int64)
    lengths = rng.integers(1, 4000, B).astype(np.int32)
    for b in range(B):
        kind = b % 8
        if kind == 1 and V >= 8:     # ties at the top-k threshold
            top = np.sort(x[b])[::-1]
            K[b] = 3
            x[b, rng.choice(V, 2, replace=False)] = top[2]
        elif kind == 2 and V >= 4:   # non-finite entries (never candidates), +inf included
            x[b, rng.choice(V, max(1, V // 20), replace=False)] = np.nan
            x[b, rng.choice(V, max(1, V // 20), replace=False)] = -np.inf
            x[b, rng.integers(V)] = np.inf
        elif kind == 3:
            lengths[b] = 0           # empty row
        elif kind == 5:              # out of domain: T < 0 / NaN -> greedy, K < 0 -> 0, P > 1 / NaN -> 1, P <= 0 -> max
            T[b], K[b], P[b] = [(-1.0, 3, 0.5), (np.nan, 0, 1.0), (0.9, -7, 2.0), (0.9, 0, np.nan), (1.2, 0, -0.5),
                                (1.2, 0, 0.0)][(b // 8) % 6]
    if B > 6 and V >= 2:
        x[6] = np.nan                # no candidate at all
        T[6] = 1.0
        lengths[6] = 5
    return x, T, K, P, seed, lengths


def check_against_reference(x, T, K, P, seed, lengths, got, what):
    want, gap, margin = ref.sample(x, T, K, P, seed, lengths)
    posed = (gap > 1e-4) & (margin > 1e-4)
    masked = ~posed
    print(f"{what}: {masked.sum()} of {len(got)} rows masked ({100.0 * masked.mean():.2f} %)")
    assert masked.mean() < 0.05
    bad = np.nonzero(posed & (got != want))[0]
    assert len(bad) == 0, f"{what}: rows {bad[:10]} got {got[bad[:10]]} want {want[bad[:10]]}"
    for b in np.nonzero(masked)[0]:   # a near tie may go either way, but never outside the kept set
        keep, _ = ref.kept_set(x[b], T[b], K[b], P[b])
        assert keep[got[b]], (what, b, got[b])
