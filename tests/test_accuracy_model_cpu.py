"""Proves on the CPU that the accuracy comparison of tests/test_attention_accuracy_gpu.py bites: for every
(family, shape) of the GPU tests, the fp32 oracle passes with its own tolerance, and nine deliberately wrong variants of
the float64 model -- the bugs attention kernels actually have -- fail the same comparer at the same tolerance by at
least 4x, in the families the table below names.  No single family sees everything; the table is asserted, so a
family that is dropped or a tolerance that is widened turns up here as a failure, without a GPU."""
import math

import numpy as np
import pytest

import f64_model as fm
from accuracy_cases import FAMILIES, SCAN_SHAPES, STREAM_CASES, apply_family, base_case, edge_lengths, oracle_scan

CHUNK = 256          # where mutants (c) and (h) cut the row
GAP = 4.0


def _f64(a):
    return np.asarray(a).astype(np.float64)


def _softmax_v(x, v):
    e = np.exp(x - x.max())
    return (e / e.sum()) @ v


# Every mutant is the float64 model of ONE row with one fault: f(qb, K [D, S], V [S, D], n, x) -> attention row, where
# x = qb . K / sqrt(D) over all S slots (dead ones included: some faults read them) is shared between the mutants.
def mutant_last_token_dropped(qb, K, V, n, x):                   # (a) masks s < L - 1
    return _softmax_v(x[:n - 1], V[:n - 1]) if n > 1 else np.zeros(V.shape[1])


def mutant_token_L_included(qb, K, V, n, x):                     # (b) reads one token past the row
    m = min(n + 1, len(x))
    return _softmax_v(x[:m], V[:m])


def mutant_first_token_of_second_chunk_dropped(qb, K, V, n, x):  # (c)
    idx = np.delete(np.arange(n), CHUNK) if n > CHUNK else np.arange(n)
    return _softmax_v(x[idx], V[idx])


def mutant_scale(qb, K, V, n, x):                                # (d) 1 / sqrt(D + 1)
    D = len(qb)
    return _softmax_v(x[:n] * math.sqrt(D / (D + 1.0)), V[:n])


def mutant_last_four_elements_missing(qb, K, V, n, x):           # (e) the row's tail never enters q . K
    return _softmax_v(x[:n] - (qb[-4:] @ K[-4:, :n]) / math.sqrt(len(qb)), V[:n])


def mutant_k_rounded_to_bf16(qb, K, V, n, x):                    # (f) an fp32 path on a reduced-precision route
    from helpers import bf16_round
    return _softmax_v((qb @ _f64(bf16_round(K[:, :n].astype(np.float32)))) / math.sqrt(len(qb)), V[:n])


def mutant_running_max_seeded_with_zero(qb, K, V, n, x):         # (g) in float32, so that the underflow is real
    x32 = x[:n].astype(np.float32)
    m = np.float32(max(0.0, float(x32.max())))
    with np.errstate(all="ignore"):
        e = np.exp(x32 - m).astype(np.float32)
        return (e @ V[:n].astype(np.float32)) / e.sum(dtype=np.float32)


def mutant_merge_without_rescale(qb, K, V, n, x):                # (h) two chunks, split at CHUNK, merged with alpha = 1
    acc, tot = np.zeros(V.shape[1]), 0.0
    for lo, hi in ([(0, CHUNK), (CHUNK, n)] if n > CHUNK else [(0, n)]):
        e = np.exp(x[lo:hi] - x[lo:hi].max())                    # the chunk's own maximum ...
        acc += e @ V[lo:hi]                                      # ... and no exp(m_chunk - m) when the partials meet
        tot += e.sum()
    return acc / tot


def mutant_probabilities_normalised_over_S(qb, K, V, n, x):      # (i) dead slots are finite and enter the sum
    e = np.exp(x - x[:n].max())
    p = np.zeros(len(x))
    p[:n] = e[:n] / e.sum()
    return p


MUTANTS = {
    "a": mutant_last_token_dropped, "b": mutant_token_L_included, "c": mutant_first_token_of_second_chunk_dropped,
    "d": mutant_scale, "e": mutant_last_four_elements_missing, "f": mutant_k_rounded_to_bf16,
    "g": mutant_running_max_seeded_with_zero, "h": mutant_merge_without_rescale, "i": mutant_probabilities_normalised_over_S,
}


def run_mutants(q, kt, v, lengths):
    """{name: [B, D] attention (probabilities [B, S] for (i))} of every mutant on a case."""
    B, D, S = kt.shape
    out = {k: np.zeros((B, S if k == "i" else D), np.float64) for k in MUTANTS}
    for b in range(B):
        n = int(lengths[b])
        if n == 0:
            continue
        qb, K, V = _f64(q[b]), _f64(kt[b]), _f64(v[b])
        x = (qb @ K) / math.sqrt(D)
        for k, fn in MUTANTS.items():
            out[k][b] = fn(qb, K, V, n, x)
    return out


# Which family catches which mutant AT EVERY SHAPE where the mutant changes anything (shapes whose rows never reach the
# second chunk cannot show (c) or (h)).  "catches" = the worst row's error is at least 4x the case's tolerance -- the
# comparison the GPU tests make.  Reasoned from the arithmetic and confirmed by running the float64 model, never from
# a kernel:
#   flat        p ~ 1 / L, every token carries weight and the tolerance is ~ 2e-6: sees everything but (g).
#   peaked      a sharper softmax: a single dropped token can carry p ~ e^-30 (a, b, c, i are shape dependent), faults of
#               the scores themselves (e, f) and of the merge (h) grow with the score range.
#   offset+/-   scores of +-200 carry an fp32 cancellation error of ~ 1e-5, which lifts the tolerance to ~ 1e-3 relative:
#               the small faults (c, d) drown, dropped / extra tokens (a, b) and wrong scores (e, f) do not.  offset- is the
#               only family in which (g) shows: exp(-200 - 0) underflows and the row is 0 / 0.
#   late_peak   the peak tokens dominate; a token outside the peak has p ~ e^-30, so (c) vanishes (1e-10 of the tolerance).
#   early_peak  likewise, and the slot at L has p ~ e^-30 against the peak: (b) and (i) vanish.  (h) is at its largest here
#               and in late_peak: the other chunk is not scaled by e^-30.
ALL = {"flat", "peaked", "offset+", "offset-", "late_peak", "early_peak"}      # spelled out: dropping a family must fail here
CATCHES = {
    "a": {"flat", "offset+", "offset-"},
    "b": {"flat", "offset+", "offset-"},
    "c": {"flat"},
    "d": {"flat"},
    "e": ALL,
    "f": ALL,
    "g": {"offset-"},
    "h": ALL,
    "i": {"flat"},
}
# ... and where a mutant must HIDE (every row within the tolerance): the reason the other families exist
MISSES = {"g": ALL - {"offset-"}, "c": {"late_peak", "early_peak"}, "b": {"early_peak"}, "i": {"early_peak"}}
# In `flat` the faults that are not about the running maximum show on EVERY long row they touch, not just on the worst
# one: the rows today's absolute 1e-3 is blind to
FLAT_EVERY_LONG_ROW = ("a", "b", "c", "d", "e", "f", "h")

# every shape of the GPU tests, B cut down (the forced edge lengths and the two long rows stay)
def _cpu_cases():
    out = []
    for seed, B, S, D, ch in SCAN_SHAPES:
        n_edges = len({e for e in [0, 1, 2, 15, 16, 17, S - 2, S - 1] + [c + k for c in ch for k in (-1, 0, 1)] if 0 <= e <= S - 1})
        out.append((seed, min(B, n_edges + 3), S, D, ch, None))
    for seed, B, S, D, lengths in STREAM_CASES:
        if isinstance(lengths, list):
            out.append((seed, B, S, D, (), lengths))
        else:
            ch = () if lengths == "short" else (64, 256)
            out.append((seed, min(B, 24), S, D, ch, lengths))
    return out


def _lengths(seed, B, S, ch, lengths):
    if isinstance(lengths, list):
        return np.asarray(lengths, np.int32)
    return edge_lengths(seed, B, S, ch, short=lengths == "short")


def _measure(oracle, seed, B, S, D, ch, lengths):
    """({family: (E_oracle, tol, {mutant: per-row errors, or None when the mutant changes nothing at this shape},
    E_oracle of the probabilities)}, lengths)"""
    L = _lengths(seed, B, S, ch, lengths)
    c = base_case(seed, B, S, D, L)
    v = c["v_cache"]
    res = {}
    for fam in FAMILIES:
        q, kt = apply_family(c, fam)
        m = fm.Model(q, kt, v, L)
        assert (m.p[m.p > 0] >= math.exp(-40)).all(), "family keeps every probability above e^-40"
        x, p, o = oracle_scan(oracle, q, kt, v, L)
        e_att = fm.attention_error(o, m).max()
        e_p = fm.probability_error(p, m).max()
        tol, tol_p = fm.tolerance(e_att), fm.tolerance(e_p)
        assert fm.attention_error(o, m).max() <= tol and e_p <= tol_p and fm.score_error(x, m).max() <= fm.tolerance(fm.score_error(x, m))
        errs = {}
        with np.errstate(all="ignore"):
            for name, got in run_mutants(q, kt, v, L).items():
                if name in ("c", "h") and L.max() <= CHUNK:
                    errs[name] = None                       # no row reaches the second chunk: the mutant changes nothing
                elif name == "i":                           # a fault of the probabilities: their metric, their tolerance,
                    errs[name] = fm.probability_error(got, m) * (tol / tol_p)   # expressed in units of the attention one
                else:
                    errs[name] = fm.attention_error(got, m)
        res[fam] = (float(e_att), tol, errs, float(e_p))
    return res, L


@pytest.mark.parametrize("seed,B,S,D,ch,lengths", _cpu_cases())
def test_oracle_passes_and_every_mutant_is_caught(oracle, seed, B, S, D, ch, lengths):
    res, L = _measure(oracle, seed, B, S, D, ch, lengths)
    assert set(res) == ALL
    for fam, (e_att, tol, errs, e_p) in res.items():
        print(f"{fam:11s} E_oracle {e_att:.2e} tol {tol:.2e} E_oracle(p) {e_p:.2e}  worst row / tol: " +
              " ".join(f"{k}={'-' if e is None else format(e.max() / tol, '.1e')}" for k, e in errs.items()))
        # tripwire for a broken model or generator: twice the largest oracle error measured when the families were designed
        assert e_att < 2e-4, (fam, e_att)
    for name in MUTANTS:
        applicable = [f for f in FAMILIES if res[f][2][name] is not None]
        if not applicable:
            continue
        caught = {f for f in applicable if not res[f][2][name].max() <= GAP * res[f][1]}     # (NaN counts as caught)
        assert CATCHES[name] <= caught, f"mutant ({name}): expected {sorted(CATCHES[name])}, caught by {sorted(caught)}"
        for f in MISSES.get(name, ()):
            assert res[f][2][name].max() <= res[f][1], f"mutant ({name}) was expected to hide in {f}"
    long_rows = L >= max(S // 2, 2)
    e_att, tol, errs, _ = res["flat"]
    for name in FLAT_EVERY_LONG_ROW:
        rows = long_rows & (L > CHUNK) if name in ("c", "h") else long_rows
        if errs[name] is not None and rows.any():
            assert (errs[name][rows] >= GAP * tol).all(), (name, errs[name][rows].min() / tol)


def test_page_gather_reads_what_the_layout_rule_wrote(oracle):
    """fill_pages (the oracle's clone through the page table) and f64_model.gather_pages (helpers.pool_index restated) are
    two statements of one layout rule: every live slot comes back as it went in, dead slots as zeros."""
    from accuracy_cases import dead_slot_offsets, fill_pages
    B, S, D = 14, 128, 64
    L = edge_lengths(5, B, S, (64,))
    c = base_case(5, B, S, D, L)
    q, kt = apply_family(c, "late_peak")
    pool, off = fill_pages(oracle, c, q, kt, c["v_cache"])
    pool[off] = np.nan
    k = fm.gather_pages(pool, c["table"], L, S, D, 1)
    v = fm.gather_pages(pool, c["table"], L, S, D, 2)
    for b in range(B):
        n = int(L[b])
        assert (k[b, :n] == kt[b, :, :n].T).all() and (v[b, :n] == c["v_cache"][b, :n]).all()
        assert not k[b, n:].any() and not v[b, n:].any()
    assert np.isnan(pool).sum() == len(off) > 0
