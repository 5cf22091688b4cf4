"""The comparison of tests/logprobs_model.py bites: the float32 restatement passes it, and each wrong generator
below misses the tolerance by replay_model.MARGIN (4 tolerances) on the score families the GPU tests use.  No GPU, no
product code: this is the check of the yardstick the kernel and engine tests are measured with."""
import numpy as np
import pytest

import logprobs_model as lm
import sampling_ref as sr
from replay_model import MARGIN

N_TOP = 8
LN2 = np.float32(np.log(2.0))


def _inputs(V):
    x, lengths = lm.families(V)
    tokens = np.array([sr.greedy(x[b]) if lengths[b] else -1 for b in range(len(x))], np.int32)
    tokens[1] = 5 % V           # a drawn token need not be the most probable one
    tokens[7] = 17 % V
    return x, tokens


def generate(x, tokens, n_top, temperature=None, subtract_max=True, log=np.log, shift=0, ascending=False, ties_high=False,
             count_non_finite=False):
    """What a head reports, evaluated in float32, with one fault switched on at a time (none: the restatement)."""
    B, V = x.shape
    tok_lp = np.full(B, -np.inf, np.float32)
    ids = np.full((B, n_top), -1, np.int64)
    lps = np.full((B, n_top), -np.inf, np.float32)
    for b in range(B):
        t = int(tokens[b])
        if t < 0:
            continue
        row = x[b] if temperature is None else (x[b] / np.float32(temperature)).astype(np.float32)
        cand = ~np.isnan(row) if count_non_finite else np.isfinite(row)
        lp = np.where(np.isneginf(row), -np.inf, np.nan).astype(np.float32)
        if cand.any():
            with np.errstate(over="ignore", invalid="ignore", under="ignore", divide="ignore"):
                m = row[cand].max() if subtract_max else np.float32(0)
                d = (row[cand] - m).astype(np.float32)
                s = np.cumsum(np.exp(d).astype(np.float32), dtype=np.float32)[-1]
                lp[cand] = (d - np.float32(log(s))).astype(np.float32)
                if not subtract_max:
                    lp[cand] = (row[cand] - np.float32(log(s))).astype(np.float32)
        tok_lp[b] = lp[t]
        c = np.nonzero(cand)[0]
        order = c[np.lexsort((-c if ties_high else c, -row[c].astype(np.float64)))][:n_top]
        if ascending:
            order = order[::-1]
        ids[b, :len(order)] = order
        lps[b, :len(order)] = lp[order]
    if shift:
        tok_lp, ids, lps = (np.roll(a, shift, axis=0) for a in (tok_lp, ids, lps))
    return tok_lp, ids, lps


@pytest.mark.parametrize("V", [1000, 15 * 1024 + 4, 5])
def test_the_float32_restatement_passes(V):
    x, tokens = _inputs(V)
    for n_top in (0, 1, 3, 8):
        err, tol, bad = lm.compare(generate(x, tokens, n_top), x, tokens, n_top)
        print(f"LOGPROBS model V {V} n_top {n_top}: restatement error {err:.3e} tol {tol:.3e}")
        assert not bad and err <= tol, (err, tol, bad)


def test_the_model_on_hand_made_rows():
    x = np.array([[0.0, np.log(3.0), -np.inf, np.log(3.0)], [np.nan, np.inf, 1.0, 1.0]], np.float32)
    lp, ids, lps = lm.reference(x, [1, 1], 3)
    np.testing.assert_allclose(lp[0], np.log(3.0 / 7.0), rtol=1e-7)
    assert ids[0].tolist() == [1, 3, 0] and ids[1].tolist() == [2, 3, -1]
    np.testing.assert_allclose(lps[0], np.log([3.0 / 7.0, 3.0 / 7.0, 1.0 / 7.0]), rtol=1e-7)
    assert np.isnan(lp[1]) and lps[1, 2] == -np.inf
    np.testing.assert_allclose(lps[1, :2], np.log(0.5), rtol=1e-7)
    lp, ids, lps = lm.reference(x, [-1, 2], 2)                     # a row that emitted nothing
    assert lp[0] == -np.inf and ids[0].tolist() == [-1, -1] and (lps[0] == -np.inf).all()
    assert lm.row_logprobs(x[0])[2] == -np.inf


MUTANTS = {
    "logprobs of the temperature-scaled distribution (T = 0.8)": dict(temperature=0.8),
    "an LSE without max subtraction": dict(subtract_max=False),
    "log2 in place of log": dict(log=np.log2),
    "figures shifted by one position against the tokens": dict(shift=1),
    "alternatives in ascending order": dict(ascending=True),
    "ties broken to the higher index": dict(ties_high=True),
    "non-finite entries counted as candidates": dict(count_non_finite=True),
}


@pytest.mark.parametrize("what", sorted(MUTANTS))
def test_the_comparison_rejects(what):
    x, tokens = _inputs(1000)
    if what == "an LSE without max subtraction":
        x, tokens = x[2:3], tokens[2:3]                 # the +-200 family is the one it breaks on
    err, tol, bad = lm.compare(generate(x, tokens, N_TOP, **MUTANTS[what]), x, tokens, N_TOP)
    print(f"LOGPROBS mutant '{what}': error {err:.3e} = {err / tol:.3g} tol ({'; '.join(bad) or 'values only'})")
    assert err >= MARGIN * tol, (what, err, tol)
