"""Proves on the CPU that the comparison of tests/test_sinks_scan_gpu.py bites (tests/sinks_model.py): on that test's own
inputs -- every shape, head count, (window, n_sink) pair and set of lengths -- the sink-windowed fp32 oracle passes against
the sink-windowed float64 model inside its own tolerance, and eight wrong models fail the same comparer at the same
tolerance by at least 4x wherever they attend other slots than the right model (the measured factors are printed):
  sinks ignored, K + 1, K - 1, K rounded up to a page, window shrunk to W - K, the gap inside a shared page attended, the
  sink mask t < K % 16 applied on every page, the sink pages read at the window's origin.
Why the inputs show them: the lengths contain K + W - 1 .. K + W + 1 and the rows whose window starts at the end of the
last sink page, on the next page edge, one slot behind it and a page further; a `flat` head moves by about 1 / (K + W) of
its value range per token added or dropped (>= 1e-3 at the largest window, against a tolerance of ~1e-6), and `early_peak`
puts its +30 tokens on slots 0 .. 15 -- on the sinks and on the gap slots that share their page.  A wrong model that attends
exactly the right slots on every row of the case is the right model there and must pass (K = 16 is a whole page: rounding
it up changes nothing).  Also: rows with lo <= K equal the un-windowed model exactly, K = 0 is the windowed model, and the
sink-aware CPU engine reproduces the window-aware one without sinks."""
import functools

import numpy as np
import pytest

import heads_model as hm
import sinks_model as sm
import window_model as wm
from accuracy_cases import base_case
from engine_sim import make_items, make_model

GAP = 4.0
CASES = [(seed, B, S, D, H, W, K, part)
         for seed, B, S, D, heads, _, pairs, _ in sm.SINK_SHAPES for W, K in pairs
         for part in range(len(sm.sink_lengths(seed, B, S, W, K))) for H in heads]
# the wrong models that attend other slots than the right one in every case with a row that has a gap
ALWAYS = ("sinks ignored", "K + 1", "K - 1", "window shrunk to W - K", "sink pages read at the window's origin")


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, W, K, part):
    return base_case(seed, B, S, D, sm.sink_lengths(seed, B, S, W, K)[part])


@pytest.mark.parametrize("assignment", hm.ASSIGNMENTS)
@pytest.mark.parametrize("seed,B,S,D,H,W,K,part", CASES)
def test_oracle_passes_and_wrong_models_fail(oracle, seed, B, S, D, H, W, K, part, assignment):
    c = _base(seed, B, S, D, W, K, part)
    q, kt = hm.apply_head_families(c, H, assignment)
    v, L = c["v_cache"], c["lengths"]
    model = sm.model_sinks(q, kt, v, L, H, W, K)
    o_or = sm.oracle_sinks(oracle, q, kt, v, L, H, W, K)
    assert (o_or[L == 0] == 0).all() and (L == 0).any()
    what = f"B{B} S{S} D{D} H{H} W{W} K{K}"
    hm.assert_within(hm.compare(o_or, o_or, model, assignment, what=f"{what} oracle"), "oracle")
    # rows without a gap are the un-windowed problem, exactly
    plain = hm.HeadsModel(q, kt, v, L, H)
    whole = wm.window_lo(L, W) <= K
    assert whole.any() and not whole.all() and np.array_equal(model.o[whole], plain.o[whole])
    assert np.array_equal(o_or[whole], hm.oracle_heads(oracle, q, kt, v, L, H)[whole])
    for name in sm.WRONG_MASKS:
        o_wrong, differs = sm.wrong_model(name, q, kt, v, L, H, W, K)
        res = hm.compare(o_wrong, o_or, model, assignment, what=f"{what} {name}")
        ratio = max(worst / tol for _, worst, tol in res)
        print(f"SINKS {what} {assignment} | {name}: misses the tolerance by {ratio:.3g}x (attends other slots: {differs})")
        if differs:
            assert ratio >= GAP, (name, assignment, ratio)
        else:
            assert ratio <= 1.0, (name, ratio)       # the same slots on every row: the right model
            assert name not in ALWAYS, name


def test_lengths_hold_the_edges_of_every_case():
    for seed, B, S, D, _, _, pairs, _ in sm.SINK_SHAPES:
        for W, K in pairs:
            assert 1 <= K and K + W < S, "every case reaches the kernels with sinks"
            L = np.concatenate(sm.sink_lengths(seed, B, S, W, K))
            have = set(L.tolist())
            for e in (0, 1, K - 1, K, K + 1, S - 1, K + W - 1, K + W, K + W + 1, W + 15, W + 16, W + 17):
                assert e in have or e > S - 1, (S, W, K, e)
            lo, skip, ps = wm.window_lo(L, W), sm.skipped_pages(L, W, K), sm.sink_pages(K)
            if S - 1 >= W + 16 * (ps + 1) + 1:
                assert ((lo // 16 == ps - 1) & (lo > 0)).any(), "lo in the last sink page"
                assert ((lo // 16 == ps) & (lo % 16 == 0)).any() and ((lo // 16 == ps) & (lo % 16 == 1)).any()
                assert (skip == 1).any()
    # the shapes together reach a hole inside a page, across a page edge, and a run of many skipped pages
    assert any(K % 16 and W + 16 * sm.sink_pages(K) - 1 <= S - 1 for *_, pairs, _ in sm.SINK_SHAPES for W, K in pairs)
    L = np.concatenate(sm.sink_lengths(503, 20, 1024, 513, 4))
    assert sm.skipped_pages(L, 513, 4).max() >= 20


def test_the_mask_is_the_contract():
    L = np.array([0, 3, 20, 21, 40, 63], np.int32)
    m = sm.sink_mask(L, 64, 16, 4)
    assert not m[0].any() and m[1, :3].all() and not m[1, 3:].any()
    assert m[2, :20].all() and m[3].sum() == 20 and not m[3, 4]              # lo = 4 = K: no gap; lo = 5: slot 4 is the gap
    assert m[4].sum() == 20 and m[4, :4].all() and m[4, 24:40].all() and not m[4, 4:24].any()
    assert m[5].sum() == 20 and m[5, 47:63].all()
    assert np.array_equal(sm.sink_mask(L, 64, 16, 0), wm.window_mask(L, 64, 16))
    assert sm.skipped_pages(L, 16, 4).tolist() == [0, 0, 0, 0, 0, 1]
    assert sm.gap_pages(L, 4, 16, 4)[5].tolist() == [False, True, False, False]


@pytest.mark.parametrize("bf16", [False, True])
def test_sinks_cpu_engine_is_the_window_cpu_engine_without_sinks(oracle, bf16):
    B, S, D, V = 8, 64, 128, 1024
    model = make_model(77, V, S, D)
    items = make_items(78, 12, 3, 20)
    for H in (1, 4):
        want, _ = wm.run_window_cpu_engine(oracle, model, items, B, S, H, 12, bf16=bf16)
        got, gap = sm.run_sinks_cpu_engine(oracle, model, items, B, S, H, 12, 0, bf16=bf16)
        assert sorted(got) == sorted(want) and np.isfinite(gap) and gap >= 0
        for k in want:
            assert np.array_equal(got[k], want[k]), k
        kept, _ = sm.run_sinks_cpu_engine(oracle, model, items, B, S, H, 12, 4, bf16=bf16)
        assert any(not np.array_equal(kept[k], want[k]) for k in want), "four sinks decode what the window alone does not"
        whole, _ = hm.run_heads_cpu_engine(oracle, model, items, B, S, H, bf16=bf16)
        full, _ = sm.run_sinks_cpu_engine(oracle, model, items, B, S, H, 12, S - 12, bf16=bf16)
        for k in whole:
            assert np.array_equal(full[k], whole[k]), k
