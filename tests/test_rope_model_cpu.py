"""tests/rope_model.py checked on the CPU: the float64 rotation against an independent complex-number formulation, the
relative-shift invariance of q_m . k_n, mli_rope_table against numpy float64, and -- the point of the file -- that the judge of
tests/test_rope_gemm_gpu.py can fail: a numpy stand-in of the epilogue passes it, and the same stand-in with one defect
(rope_model.DEFECTS) is rejected, each by name.  No GPU."""
import ctypes

import numpy as np
import pytest

import gemm_model as gm
import rope_model as rp


def _complex_rotate(y, slots, table, n_heads):
    """pair i of head h as the complex number y[2i] + j y[2i + 1], multiplied by c + j sn"""
    R, D = y.shape
    hd = D // n_heads
    z = y.reshape(R, n_heads, hd // 2, 2).astype(np.float64)
    z = z[..., 0] + 1j * z[..., 1]
    t = np.asarray(table, np.float32).astype(np.float64)[np.asarray(slots)]
    w = (t[..., 0] + 1j * t[..., 1])[:, None, :]
    out = z * w
    return np.stack([out.real, out.imag], axis=-1).reshape(R, D)


@pytest.mark.parametrize("D,H", [(128, 1), (128, 4), (66, 1), (96, 3)])
def test_the_model_is_a_complex_multiplication(D, H):
    rng = np.random.default_rng(D + H)
    S = 200
    y = rng.standard_normal((50, D))
    slots = rng.integers(0, S, size=50)
    table = rp.standard_table(S, D // H)
    assert np.abs(rp.rotate(y, slots, table, H) - _complex_rotate(y, slots, table, H)).max() <= 4 * 2.0 ** -52 * np.abs(y).max()
    assert (rp.rotate(y, slots, rp.identity_table(S, D // H), H) == y).all()
    # the epilogue's own arithmetic hands an identity entry's element back bit for bit
    y32 = y.astype(np.float32)
    assert (rp.rotate(y32, slots, rp.identity_table(S, D // H), H, dtype=np.float32).view(np.uint32) == y32.view(np.uint32)).all()


def test_scores_depend_on_the_distance_alone():
    """q_m . k_n under the rotation equals q_(m + d) . k_(n + d): exact on a table of exact angles, so the table is built in
    float64 here (the fp32 table's own rounding is an input error, not the model's)."""
    rng = np.random.default_rng(5)
    D, H, S = 64, 2, 512
    hd = D // H
    i = np.arange(hd // 2)
    ang = np.arange(S)[:, None] * np.power(10000.0, -2.0 * i / hd)[None, :]

    def rot(y, s):
        z = (y.reshape(H, hd // 2, 2)[..., 0] + 1j * y.reshape(H, hd // 2, 2)[..., 1]) * np.exp(1j * ang[s])[None, :]
        return np.stack([z.real, z.imag], -1).reshape(D)

    q, k = rng.standard_normal(D), rng.standard_normal(D)
    for m, n, d in [(10, 3, 0), (10, 3, 400), (255, 255, 100), (17, 0, 494)]:
        for h in range(H):
            sl = slice(h * hd, (h + 1) * hd)
            a, b = rot(q, m)[sl] @ rot(k, n)[sl], rot(q, m + d)[sl] @ rot(k, n + d)[sl]
            assert abs(a - b) <= 1e-11 * (np.abs(q[sl]) @ np.abs(k[sl]))
    # and the model itself, on the fp32 table, to the table's own rounding
    table = rp.standard_table(S, hd)
    a = rp.rotate(q[None], [10], table, H)[0] @ rp.rotate(k[None], [3], table, H)[0]
    b = rp.rotate(q[None], [410], table, H)[0] @ rp.rotate(k[None], [403], table, H)[0]
    assert abs(a - b) <= 8 * 2.0 ** -24 * (np.abs(q) @ np.abs(k))


@pytest.mark.parametrize("S,hd,theta", [(64, 32, 10000.0), (4096, 128, 10000.0), (300, 2, 500000.0), (17, 66, 1e6)])
def test_mli_rope_table_is_the_numpy_table(mli, S, hd, theta):
    out = np.full((S, hd // 2, 2), np.nan, np.float32)
    assert mli.mli_rope_table(S, hd, theta, out.ctypes.data_as(ctypes.c_void_p)) == 0
    want = rp.standard_table(S, hd, theta)
    assert np.abs(out.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -24
    assert (out[0, :, 0] == 1.0).all() and (out[0, :, 1] == 0.0).all(), "slot 0 is the identity, exactly"
    s = np.arange(S, dtype=np.float64)
    assert (out[:, 0, 0] == np.cos(s).astype(np.float32)).all() or np.abs(out[:, 0, 0] - np.cos(s)).max() <= 2.0 ** -24
    assert np.abs(out[:, 0, 1] - np.sin(s)).max() <= 2.0 ** -24
    from min_llm_inference_amd import ops
    assert (ops.rope_table(S, hd, theta).view(np.uint32) == out.view(np.uint32)).all()


# ---- the judge can fail ---------------------------------------------------------------------------------------------------------------
H = 4
LATEST_L = [0, 1, 16, 17, 64, 33, 5, 0, 40, 64, 2, 63]


def _latest(fmt):
    c = gm.Case(901, "paged", fmt, "signed", len(LATEST_L), 64, 128, 128, LATEST_L)
    return c, "latest", 0, 0


def _fill(fmt):
    (c, mode) = gm.fill_case(902, fmt, "signed", 8, 128, 128)
    return c, mode, 0, 0


def _live_fill(fmt):
    rng = np.random.default_rng(903)
    L = np.array([100, 20, 0, 100, 50, 7], np.int32)
    c = gm.Case(903, "paged", fmt, "signed", 6, 128, 128, 128, L, rng.permutation(6).astype(np.int32), 6, vocab=40)
    return c, "prefill", 32, 4


# which case shows which defect: a position defect needs the form whose position it confuses
CASES = {"latest": _latest, "fill": _fill, "live": _live_fill}
WHERE = {"sign of sn flipped": ("latest", "fill"), "pairs (2i + 1, 2i + 2)": ("latest", "fill"), "half-split pairing": ("latest", "fill"),
         "frequency index n / 2": ("latest", "fill"), "position L": ("latest",), "flat-list index as position": ("fill",),
         "live index as position": ("live",), "V rotated as well": ("latest", "fill", "live"), "q not rotated": ("latest",)}


def _judged(oracle, built, fmt, defect):
    c, mode, W, K = built
    table = rp.standard_table(c.S, c.Din // H)
    e = rp.Expect(oracle, c, mode, table, H, W, K)
    after, q_after = rp.restate(c, e, defect, W, K)
    fig = gm.Figures(f"{mode} {fmt} [{defect}]")
    rp.judge(fig, c, e, after, q_after)
    return fig


@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("case", ["latest", "fill", "live"])
def test_the_stand_in_passes(oracle, fmt, case):
    fig = _judged(oracle, CASES[case](fmt), fmt, None)
    fig.done()
    assert len(fig.records) >= 2


@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("defect", [d for d in rp.DEFECTS if d != "rotation after the rounding"])
def test_every_defect_is_rejected(oracle, fmt, defect):
    for case in WHERE[defect]:
        fig = _judged(oracle, CASES[case](fmt), fmt, defect)
        assert fig.failures, f"{defect} passes the judge on the {case} case ({fmt})"
        named = "V (" if defect == "V rotated as well" else ("q rotated" if defect == "q not rotated" else "K rotated")
        assert any(named in f for f in fig.failures), fig.failures


@pytest.mark.parametrize("case", ["latest", "fill"])
def test_rotation_after_the_bf16_rounding_is_rejected(oracle, case):
    """K rounded to bf16, rotated, and rounded again misses by up to a bf16 half step of a and of b beyond the one half step the
    judge takes off: 2^-9 at |a| ~ 1 against a bound of some 10^-5."""
    fig = _judged(oracle, CASES[case]("bf16"), "bf16", "rotation after the rounding")
    assert any("K rotated" in f for f in fig.failures), fig.failures
    assert not any("V (" in f or "q rotated" in f for f in fig.failures), fig.failures


def test_the_live_fill_case_has_dead_pages():
    c, mode, W, K = _live_fill("f32")
    full = gm.fill_rows(c.new_idx[:c.n_new], c.L)
    e = rp.Expect(None, c, mode, rp.standard_table(c.S, c.Din // H), H, W, K)
    assert 0 < len(e.rows) < len(full)
    assert any(rp.live_index(s, int(c.L[b]), W, K) != s for b, s in e.rows)
    assert [rp.live_index(s, 100, W, K) for s in (0, 15, 64, 99)] == [0, 15, 16, 51]     # pages 1 .. 3 of a 100-token row are dead


# ---- the engine replay with the rotation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", ["f32", "bf16"])
def test_the_rotated_replay_accepts_its_own_streams_and_rejects_others(store):
    import replay_model as rm
    from engine_sim import make_items, make_model
    S, D, V, Hh = 64, 128, 1024, 4
    model = make_model(8648, V, S, D)
    model["pos_table"] = np.zeros_like(model["pos_table"])      # a RoPE model has no learned positions
    items = make_items(9648, 6, 3, 20)
    table = rp.standard_table(S, D // Hh)
    spec = rp.rope_spec(rm.Spec(store, Hh, None, 0, False), table)
    right = [(i, rp.generate(model, t, spec, S)) for i, t in items]
    rp.audit(model, items, right, spec, S, what=f"rotated replay {store}").assert_ok()
    # with an identity table the rotated replay IS replay_model's
    ident = rp.rope_spec(rm.Spec(store, Hh, None, 0, False), rp.identity_table(S, D // Hh))
    for i, t in items[:2]:
        toks = rp.generate(model, t, ident, S)
        a = rp.RopeReplay(model, toks, ident).logits
        b = rm.Replay(model, toks, rm.Spec(store, Hh, None, 0, False)).logits
        assert (a == b).all()
    # an engine that does not rotate, one that rotates by position + 1 (q and K alike: invisible, the scores depend on the
    # distance alone) and one that rotates K by position + 1 only
    plain = [(i, rp.generate(model, t, spec, S, wrong_table=rp.identity_table(S, D // Hh))) for i, t in items]
    fig = rp.audit(model, items, plain, spec, S, what=f"an engine without the rotation {store}", report=lambda s: None)
    assert fig.failures, "the audit does not see an engine that never rotates"
    assert any(len(a[1]) != len(b[1]) or (a[1] != b[1]).any() for a, b in zip(right, plain))
