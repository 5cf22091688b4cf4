"""The ALiBi test infrastructure (tests/alibi_model.py) and mli_alibi_slopes, without a GPU:
  - mli_alibi_slopes against an independent numpy restatement for 2 .. 32 heads, and against the values everybody quotes;
  - the float64 model with slopes all zero IS gqa_model.model_gqa, plain, windowed and with sinks;
  - every wrong model misses the tolerance by at least 4 x on inputs chosen for it (flat q . K scores, the standard slopes),
    while the float32 evaluation of the right model stays inside the tolerance on those inputs: the comparison the GPU tests
    make bites;
  - the replay audit with the bias accepts a stream decoded on its own forward and rejects one decoded without the bias."""
import ctypes

import numpy as np
import pytest

import alibi_model as am
import gqa_model as gm
import heads_model as hm
from helpers import paged_case

MARGIN = 4.0


def _slopes(mli, H):
    out = np.full(H, np.nan, np.float32)
    assert mli.mli_alibi_slopes(H, out.ctypes.data_as(ctypes.c_void_p)) == 0
    return out


def test_standard_slopes(mli):
    for H in range(2, 33):
        got = _slopes(mli, H)
        assert got.dtype == np.float32 and np.array_equal(got, am.standard_slopes(H)), H
        assert np.isfinite(got).all() and (got > 0).all() and (got < 1).all(), H
    assert np.array_equal(_slopes(mli, 8), np.float32(2.0) ** -np.arange(1, 9))
    assert np.array_equal(_slopes(mli, 3), np.asarray([1 / 16, 1 / 256, 1 / 4], np.float32))
    assert np.array_equal(_slopes(mli, 12)[-4:], (2.0 ** -np.asarray([0.5, 1.5, 2.5, 3.5])).astype(np.float32))
    assert np.array_equal(_slopes(mli, 1), np.asarray([2.0 ** -8], np.float32))
    from min_llm_inference_amd import ops
    assert np.array_equal(ops.alibi_slopes(12), _slopes(mli, 12))


def test_bad_slope_requests_are_refused(mli):
    out = np.zeros(4, np.float32)
    for H in (0, -1):
        assert mli.mli_alibi_slopes(H, out.ctypes.data_as(ctypes.c_void_p)) == -22
    assert mli.mli_alibi_slopes(4, None) == -22
    assert not out.any()


def _case(seed, B, S, D, lengths):
    c = paged_case(seed, B, S, D, conditioned=True, lengths=np.asarray(lengths, np.int32))
    return c["q_output"], c["kt_cache"], c["v_cache"], c["lengths"]


@pytest.mark.parametrize("W,K", [(0, 0), (40, 0), (5, 0), (40, 4), (40, 20)])
def test_zero_slopes_are_the_grouped_query_model(W, K):
    q, kt, v, L = _case(7101, 8, 128, 128, [0, 1, 16, 17, 45, 64, 100, 128])
    for H, Hkv in ((4, 4), (4, 2), (4, 1)):
        want = gm.model_gqa(q, kt, v, L, H, Hkv, W, K)
        got = am.AlibiModel(q, kt, v, L, H, Hkv, np.zeros(H, np.float32), W, K)
        assert np.abs(got.o - want.o).max() < 1e-14 and np.abs(got.o_scale - want.o_scale).max() < 1e-14, (H, Hkv)
        assert (got.o[0] == 0).all()


# (what, B, S, D, H, Hkv, W, K, epl, lengths): the inputs on which the fault shows -- rows of several pages, of several items,
# with a skipped page under sinks, grouped heads, rows of two lane loads
WRONG_CASES = {
    "slopes ignored": (6, 128, 128, 4, 4, 0, 0, 4, [2, 17, 40, 64, 100, 128]),
    "sign flipped": (6, 128, 128, 4, 4, 0, 0, 4, [2, 17, 40, 64, 100, 128]),
    "slope of head h + 1": (6, 128, 128, 4, 2, 40, 0, 4, [2, 17, 40, 64, 100, 128]),
    "slope of the K/V head": (6, 128, 128, 4, 2, 0, 0, 4, [2, 17, 40, 64, 100, 128]),
    "position inside the page": (6, 128, 128, 4, 4, 0, 0, 4, [17, 33, 40, 64, 100, 128]),
    "position restarts at every item": (6, 256, 128, 4, 4, 0, 0, 4, [65, 100, 129, 200, 255, 256]),
    "gap under sinks not counted": (6, 256, 128, 4, 4, 40, 4, 4, [80, 100, 129, 200, 255, 256]),
    "first lane load's slope for both": (6, 128, 512, 8, 8, 0, 0, 4, [2, 17, 40, 64, 100, 128]),
}
assert set(WRONG_CASES) == set(am.WRONG)


@pytest.mark.parametrize("name", am.WRONG)
def test_every_wrong_model_misses_the_tolerance(name):
    B, S, D, H, Hkv, W, K, epl, lengths = WRONG_CASES[name]
    q, kt, v, L = _case(7200 + am.WRONG.index(name), B, S, D, lengths)
    slopes = am.standard_slopes(H)
    model = am.AlibiModel(q, kt, v, L, H, Hkv, slopes, W, K)
    o32 = am.eval_fp32(q, kt, v, L, H, Hkv, slopes, W, K)
    tol = am.tolerance(model, o32)
    e32 = float(hm.heads_error(o32, model).max())
    bad = float(hm.heads_error(am.wrong(name, q, kt, v, L, H, Hkv, slopes, W, K, epl), model).max())
    print(f"ALIBI wrong model '{name}': error {bad:.3e}, tolerance {tol:.3e} (float32 evaluation of the right model {e32:.3e})")
    assert e32 <= tol < 1e-5
    assert bad >= MARGIN * tol, name


def test_the_lane_load_fault_needs_rows_of_two_lane_loads():
    """on rows of one lane load every head takes its own slope: the wrong model is the right one there"""
    assert [am.lane_load_head(h, 4, 128, 4) for h in range(4)] == [0, 1, 2, 3]
    assert [am.lane_load_head(h, 8, 512, 4) for h in range(8)] == [0, 1, 2, 3, 0, 1, 2, 3]
    assert [am.lane_load_head(h, 16, 1024, 8) for h in range(16)] == list(range(8)) * 2


def test_the_audit_with_the_bias_accepts_its_own_stream_and_rejects_one_without():
    from engine_sim import make_items, make_model
    S, D, V, H = 64, 128, 1024, 4
    model, items = make_model(8648, V, S, D), make_items(9648, 6, 3, 20)
    slopes = tuple(float(m) for m in am.standard_slopes(H))
    spec = am.AlibiSpec("f32", H, None, 0, False, slopes)
    right = [(i, am.generate(model, p, spec, S)) for i, p in items]
    am.audit(model, items, right, spec, S, what="the ALiBi forward's own stream").assert_ok()
    plain = [(i, am.generate(model, p, spec, S, wrong_slopes=(0.0,) * H)) for i, p in items]
    assert any(len(a) != len(b) or (a != b).any() for (_, a), (_, b) in zip(right, plain)), "the bias changes no token"
    fig = am.audit(model, items, plain, spec, S, what="a stream decoded without the bias")
    assert fig.failures and not fig.bookkeeping
    assert fig.worst_ratio >= MARGIN, fig.line()
