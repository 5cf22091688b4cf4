"""The GEMM comparer of tests/gemm_model.py can fail (GEMM block), proved without a GPU: a numpy restatement of a
tiled GEMM (64 x 64 tiles, 32-deep k slabs, fp32 accumulation) with the kernels' scatter goes through exactly the judge, the
metrics and the tolerances of tests/test_gemm_edges_gpu.py.  Unmutated it passes on a representative subset of that file's
inputs -- which is also where the CPU run confirms that the oracle alone stays inside every bound (judge checks the
oracle's rounded values against the bound they set, and every tolerance is computed from the oracle) -- and each of the
listed wrong variants fails."""
import numpy as np
import pytest

import gemm_model as gm


_latest, _fill = gm.latest_case, gm.fill_case


# a subset of the GPU grid's inputs: every format, layout and mode; ragged and full tiles; k tails 4, 28, 8, 0
REPRESENTATIVE = {
    "f32-latest-B65-D68": lambda: _latest(1, "f32", "signed", 65, 48, 68),
    "f32-latest-B129-D260-positive": lambda: _latest(2, "f32", "positive", 129, 32, 260),
    "f32-fill-D60": lambda: _fill(3, "f32", "signed", 12, 80, 60),
    "f32-prefill-D68": lambda: _fill(4, "f32", "signed", 12, 80, 68, mode="prefill"),
    "naive-latest-101x257": lambda: _latest(5, "f32", "signed", 65, 100, 101, layout="naive", Dout=257),
    "naive-fill-64x68": lambda: _fill(6, "f32", "signed", 12, 100, 64, layout="naive", Dout=68),
    "naive-prefill-260x64": lambda: _fill(7, "f32", "signed", 9, 128, 260, layout="naive", Dout=64, mode="prefill"),
    "bf16-latest-B65-D72": lambda: _latest(8, "bf16", "signed", 65, 48, 72),
    "bf16-fill-D264": lambda: _fill(9, "bf16", "signed", 12, 80, 264),
    "bf16-latest-B129-D56-positive": lambda: _latest(10, "bf16", "positive", 129, 32, 56),
    "fp8-latest-B65-D80": lambda: _latest(11, "fp8", "signed", 65, 48, 80),
    "fp8-fill-D48": lambda: _fill(12, "fp8", "signed", 12, 80, 48),
    "fp8-prefill-D80-saturating": lambda: _fill(13, "fp8", "signed", 12, 80, 80, mode="prefill", saturate=True),
    "fp8-latest-B200-D272-positive": lambda: _latest(14, "fp8", "positive", 200, 32, 272),
}


def _failures(oracle, key, mutant=None):
    c, mode = REPRESENTATIVE[key]()
    e = gm.Expect(oracle, c, mode)
    after, q_after = gm.restate(c, e, mutant)
    return gm.judge(gm.Figures(f"{key} [{mutant}]"), c, e, after, q_after).failures


@pytest.mark.parametrize("key", sorted(REPRESENTATIVE))
def test_the_restated_gemm_and_the_oracle_pass(oracle, key):
    assert _failures(oracle, key) == []


def test_oracle_product_is_the_oracles_projection_loop(oracle):
    """gemm_model.oracle_product (oracle_gemm_transpose on the gathered rows) gives the bits of oracle_get_latest_kt_q_v and
    oracle_fill_new_kt_v_cache: it is the oracle, not a third evaluation."""
    c, _ = _fill(21, "f32", "signed", 9, 48, 36, layout="naive", Dout=44)
    kt, v, q = c.kt.copy(), c.v.copy(), c.q.copy()
    oracle.get_latest_kt_q_v(c.inp, c.L, c.w["wk"], c.w["wq"], c.w["wv"], kt, v, q)
    e = gm.Expect(oracle, c, "latest")
    bb, ss = np.array([r[0] for r in e.rows]), np.array([r[1] for r in e.rows])
    assert (kt[bb, :, ss] == e.oracle["wk"]).all() and (v[bb, ss] == e.oracle["wv"]).all() and (q[bb] == e.oracle["wq"]).all()
    oracle.fill_new_kt_v_cache(c.inp, c.new_idx, c.L, c.w["wk"], c.w["wv"], kt, v, c.n_new)
    e = gm.Expect(oracle, c, "fill")
    bb, ss = np.array([r[0] for r in e.rows]), np.array([r[1] for r in e.rows])
    assert len(bb) and (kt[bb, :, ss] == e.oracle["wk"]).all() and (v[bb, ss] == e.oracle["wv"]).all()


# mutant -> the cases that must see it (every mutant on every format it applies to)
MUTANTS = {
    "drop_last_slab": ["f32-latest-B65-D68", "f32-fill-D60", "bf16-fill-D264", "fp8-latest-B65-D80", "naive-latest-101x257"],
    "double_slab": ["f32-latest-B129-D260-positive", "bf16-latest-B65-D72", "fp8-fill-D48", "naive-fill-64x68"],
    "skip_last_col_tile": ["f32-latest-B65-D68", "bf16-fill-D264", "fp8-latest-B65-D80", "naive-latest-101x257"],
    "last_row_tile_off_by_one": ["f32-latest-B65-D68", "f32-fill-D60", "bf16-latest-B65-D72", "fp8-fill-D48", "naive-fill-64x68"],
    "swap_rows": ["f32-latest-B65-D68", "bf16-fill-D264", "fp8-latest-B65-D80", "naive-prefill-260x64"],
    "toward_zero": ["bf16-latest-B65-D72", "bf16-fill-D264", "fp8-latest-B65-D80", "fp8-fill-D48"],
    "no_saturation": ["fp8-prefill-D80-saturating"],
    "empty_row_q": ["f32-latest-B65-D68", "bf16-latest-B65-D72", "fp8-latest-B65-D80", "naive-latest-101x257"],
    "stray_byte": ["f32-latest-B65-D68", "bf16-fill-D264", "fp8-fill-D48", "naive-fill-64x68"],
    "fill_stops_short": ["f32-fill-D60", "bf16-fill-D264", "fp8-fill-D48", "naive-fill-64x68", "f32-prefill-D68"],
    "fill_writes_token_L": ["f32-fill-D60", "bf16-fill-D264", "fp8-fill-D48", "naive-fill-64x68"],
    "compact_restart": ["f32-fill-D60", "bf16-fill-D264", "fp8-fill-D48", "naive-fill-64x68"],
}


@pytest.mark.parametrize("mutant,key", [(m, k) for m in MUTANTS for k in MUTANTS[m]])
def test_every_mutant_fails_the_judge(oracle, mutant, key):
    failures = _failures(oracle, key, mutant)
    assert failures, f"{mutant} passes on {key}: the comparison is blind to it"


def test_the_saturating_case_saturates(oracle):
    """The fp8 prefill case feeds +-448 to the product and has results beyond the format's range (else the unsaturated
    store would have nothing to get wrong)."""
    c, mode = REPRESENTATIVE["fp8-prefill-D80-saturating"]()
    e = gm.Expect(oracle, c, mode)
    assert (np.abs(e.x) == 448).sum() >= c.Din // 8 and np.abs(e.x).max() == 448
    assert (np.abs(e.want["wk"]) > 464).any() or (np.abs(e.want["wv"]) > 464).any()


def test_rounding_toward_zero_is_seen_at_the_half_step():
    """stored_error takes exactly half a step off: a value rounded to nearest has error 0 against itself, the neighbour
    code (a full step away, what truncation gives for the upper half of every interval) has not."""
    y = np.array([[1.0 + 2.0 ** -9, 300.0, -0.3, 2.0 ** -8]])
    scale = np.array([1.0])
    for fmt in ("bf16", "fp8"):
        near = gm.round_to(y.astype(np.float32), fmt)
        assert gm.stored_error(near, y, scale, fmt)[0] == 0.0
        step = 2 * gm.half_step(near, fmt)
        assert gm.stored_error(near + step, y, scale, fmt)[0] > 0.0
        assert gm.stored_error(near - step, y, scale, fmt)[0] > 0.0
    assert gm.stored_error(np.array([[np.nan]]), np.array([[1.0]]), scale, "fp8")[0] == np.inf
    assert gm.stored_error(np.array([[448.0]]), np.array([[1e6]]), scale, "fp8")[0] == 0.0   # saturation is the contract


@pytest.mark.parametrize("seed,family,B,V,D", [(31, "signed", 65, 33, 36), (32, "positive", 33, 1030, 36), (33, "signed", 129, 65, 260),
                                                (34, "signed", 1, 1, 4)])
def test_logits_judge_passes_the_oracle_and_fails_a_skipped_vocabulary_row(oracle, seed, family, B, V, D):
    c = gm.LogitsCase(seed, family, B, V, D)
    score = gm.oracle_product(oracle, c.att, c.emb.T)
    tokens = np.where(c.L > 0, np.argmax(score, axis=1), -1)
    fig = gm.Figures("oracle logits")
    gm.judge_logits(fig, oracle, c, score, tokens, tokens)
    assert fig.failures == []
    # the vocabulary's last row skipped: its column keeps what memory held, and rows it would have won pick another token
    bad = score.copy()
    bad[:, V - 1] = c.score0[:, V - 1]
    fig = gm.Figures("last vocabulary row skipped")
    gm.judge_logits(fig, oracle, c, bad, tokens)
    assert fig.failures
    if V >= 4:   # the tie goes to the higher index
        wrong = tokens.copy()
        wrong[tokens == 1] = V - 1
        assert (tokens == 1).any()
        fig = gm.Figures("tie to the higher index")
        gm.judge_logits(fig, oracle, c, score, wrong)
        assert fig.failures
