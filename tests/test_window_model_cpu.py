"""Proves on the CPU that the comparison of tests/test_window_scan_gpu.py bites (tests/window_model.py): on that test's own
inputs -- every shape, head count, window and set of lengths -- the windowed fp32 oracle passes against the windowed
float64 model inside its own tolerance, and six wrong models of the window fail the same comparer at the same tolerance
by at least 4x (the measured factors are printed):
  window ignored, lo one too low (W + 1 tokens), lo one too high, newest token excluded (window [lo - 1, L - 1)),
  page-granular window (lo rounded down to a page start), the first page's low mask applied to every page of the row.
Why the inputs show them: the lengths contain W - 1 .. W + 17, so there are rows just longer than the window whose first
live page is cut 1, 15 and 0 slots in; a `flat` head moves by about 1 / W of its value range per token added or dropped
(>= 1e-3 at the largest window, against a tolerance of ~1e-6), and `early_peak` puts its +30 tokens outside the window of
every row longer than W + 16, where "window ignored" is gross.  A wrong model that attends exactly the window on every
row of the case is the right model there and must pass: that happens only where no row is longer than the window
(W = 255 at n_sequence 256: lengths end at 255) or where the window starts on a page edge in every longer row.
Also: rows with L <= W equal the un-windowed model exactly, and the window-aware CPU engine reproduces the head-aware one
when the window covers the sequence."""
import functools

import numpy as np
import pytest

import heads_model as hm
import window_model as wm
from accuracy_cases import base_case
from engine_sim import make_items, make_model

GAP = 4.0
CASES = [(seed, B, S, D, H, W, chunks, part)
         for seed, B, S, D, heads, _, windows, _, chunks in wm.WINDOW_SHAPES for W in windows
         for part in range(len(wm.window_lengths(seed, B, S, W, chunks))) for H in heads]


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, W, chunks, part):
    return base_case(seed, B, S, D, wm.window_lengths(seed, B, S, W, chunks)[part])


@pytest.mark.parametrize("assignment", hm.ASSIGNMENTS)
@pytest.mark.parametrize("seed,B,S,D,H,W,chunks,part", CASES)
def test_oracle_passes_and_wrong_models_fail(oracle, seed, B, S, D, H, W, chunks, part, assignment):
    c = _base(seed, B, S, D, W, chunks, part)
    q, kt = hm.apply_head_families(c, H, assignment)
    v, L = c["v_cache"], c["lengths"]
    model = wm.model_window(q, kt, v, L, H, W)
    o_or = wm.oracle_window(oracle, q, kt, v, L, H, W)
    assert (o_or[L == 0] == 0).all() and (L == 0).any()
    what = f"B{B} S{S} D{D} H{H} W{W}"
    hm.assert_within(hm.compare(o_or, o_or, model, assignment, what=f"{what} oracle"), "oracle")
    # rows the window does not cut are the un-windowed problem, exactly
    plain = hm.HeadsModel(q, kt, v, L, H)
    short = L <= W
    assert short.any() and np.array_equal(model.o[short], plain.o[short])
    assert np.array_equal(o_or[short], hm.oracle_heads(oracle, q, kt, v, L, H)[short])
    for name in wm.WRONG_MASKS:
        o_wrong, differs = wm.wrong_model(name, q, kt, v, L, H, W)
        res = hm.compare(o_wrong, o_or, model, assignment, what=f"{what} {name}")
        ratio = max(worst / tol for _, worst, tol in res)
        print(f"WINDOW {what} {assignment} | {name}: misses the tolerance by {ratio:.3g}x (attends other slots: {differs})")
        if differs:
            assert ratio >= GAP, (name, assignment, ratio)
        else:
            assert ratio <= 1.0, (name, ratio)       # the same slots on every row: the right model
            assert L.max() <= W or name in ("page-granular window", "low mask on every page"), name
    if L.max() > W:
        for name in ("window ignored", "lo one too low", "lo one too high", "newest token excluded"):
            assert wm.wrong_model(name, q, kt, v, L, H, W)[1], name


def test_lengths_hold_the_edges_of_every_case():
    for seed, B, S, D, _, _, windows, _, chunks in wm.WINDOW_SHAPES:
        for W in windows:
            parts = wm.window_lengths(seed, B, S, W, chunks)
            have = set(np.concatenate(parts).tolist())
            assert {0, S - 1, W - 1, W}.issubset(have | {-1, S})
            for e in (W + 1, W + 15, W + 16, W + 17):
                assert e in have or e > S - 1, (S, W, e)
            if S - 1 >= W + 17:     # both kinds of wrong first page are visible
                lo = wm.window_lo(np.concatenate(parts), W)
                assert (lo % 16 != 0).any() and ((lo > 0) & (lo % 16 == 0)).any()


def test_slicing_moves_the_window_to_the_front():
    rng = np.random.default_rng(5)
    kt = rng.standard_normal((3, 4, 32)).astype(np.float32)
    v = rng.standard_normal((3, 32, 4)).astype(np.float32)
    L = np.array([0, 7, 30], np.int32)
    kt2, v2, L2 = wm.window_slice(kt, v, L, 10)
    assert L2.tolist() == [0, 7, 10]
    assert np.array_equal(kt2[2, :, :10], kt[2, :, 20:30]) and np.array_equal(v2[2, :10], v[2, 20:30])
    assert np.array_equal(kt2[1, :, :7], kt[1, :, :7]) and not kt2[2, :, 10:].any() and not v2[0].any()


@pytest.mark.parametrize("bf16", [False, True])
def test_window_cpu_engine_is_the_heads_cpu_engine_without_a_window(oracle, bf16):
    B, S, D, V = 8, 64, 128, 1024
    model = make_model(77, V, S, D)
    items = make_items(78, 12, 3, 20)
    for H in (1, 4):
        want, _ = hm.run_heads_cpu_engine(oracle, model, items, B, S, H, bf16=bf16)
        got, gap = wm.run_window_cpu_engine(oracle, model, items, B, S, H, S, bf16=bf16)
        assert sorted(got) == sorted(want) and np.isfinite(gap) and gap >= 0
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        cut, _ = wm.run_window_cpu_engine(oracle, model, items, B, S, H, 12, bf16=bf16)
        assert any(not np.array_equal(cut[k], want[k]) for k in want), "a window of 12 decodes what no window decodes"
