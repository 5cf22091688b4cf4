"""Proves without a GPU that the sink-logit comparisons of tests/test_shape_limits_gpu.py and tests/test_prompt_long_gpu.py bite
("the frontier"): limit_cases.row_truth with `sink` is sink_logits_model's float64 model on a dense case; on the small
siblings of the GPU cases -- the same generators with fewer rows -- limit_cases.judge_rows(..., sink=z) accepts the float32
evaluation of the expression and rejects every applicable wrong model of sink_logits_model.WRONG evaluated on the sparse rows;
the sink's float64 share lies in sink_logits_model.SHARE_BAND on at least MIN_BITING of the judged (row, head) pairs of every
case (limit_cases.biting), with the logits the GPU tests take (limit_cases.learned_sparse: per head, the median log-sum-exp of
the judged rows plus the per-head offset).

A wrong model that cannot differ from the right one on a case (no grouping, no window, one lane load, a single item) is listed
in the case's INAPPLICABLE set, which is asserted: none is skipped silently.

"maximum over the scores only" is the same function as the right model wherever z - max x stays inside float32's expf range,
so it is judged as tests/test_sink_logits_model_cpu.py judges it: at a logit FAR_ABOVE the largest score, against the float64
model at that logit, with the tolerance of the learned launch."""
import contextlib
from types import SimpleNamespace

import numpy as np
import pytest

import f64_model as fm
import limit_cases as lc
import prompt_model as pm
import sink_logits_model as sl

FAR = "maximum over the scores only"


def _tolerances(res):
    return {f: (max(e), fm.tolerance(np.asarray(o))) for f, (e, o) in res.items()}


def _float32_evaluation(oracle, case, values_of, rows, H, Hkv, W, K, z):
    got = np.zeros((case.B, case.D), np.float32)
    for b in rows:
        if case.lengths[b]:
            Kb, Vb = values_of(b)
            for cols, _, (_, _, o) in lc.row_truth(oracle, case.q[b], Kb, Vb, H, Hkv, W, K, sink=z):
                got[b, cols] = o[0]
    return got


def _wrong_rows(name, case, values_of, rows, H, Hkv, W, K, z, epl):
    """sink_logits_model.wrong on the sparse rows, one row at a time"""
    got = np.zeros((case.B, case.D), np.float64)
    for b in rows:
        n = int(case.lengths[b])
        if n:
            Kb, Vb = values_of(b)
            got[b] = sl.wrong(name, case.q[b][None], np.ascontiguousarray(Kb.T)[None], Vb[None], [n], H, Hkv, z, W, K, epl)[0]
    return got


@contextlib.contextmanager
def _items_of(tokens):
    """sink_logits_model counts "once per item" by ITEM_TOKENS: the item size of the case under test"""
    keep = sl.ITEM_TOKENS
    sl.ITEM_TOKENS = tokens
    try:
        yield
    finally:
        sl.ITEM_TOKENS = keep


def _applicable(name, case, rows, H, Hkv, W, D, epl, item):
    n = max(len(lc.attended(int(case.lengths[b]), W, 0)) for b in rows)
    return {"logit of the K/V head": Hkv < H, "sink counted once per item": n > item,
            "sink dropped where a window is active": W > 0 and max(int(case.lengths[b]) for b in rows) > W,
            "one lane load only": any(sl.second_lane_load(h, H, D, epl) for h in range(H))}.get(name, True)


def _proof(oracle, case, values_of, rows, H, Hkv, W, K, what, epl=4, item=64, inapplicable=(), largest=None):
    lse = lc.judged_lse(case, values_of, rows, H, Hkv, W, K)
    z = lc.learned_sparse(lse)
    f = lc.biting(lse, z, what)
    o32 = _float32_evaluation(oracle, case, values_of, rows, H, Hkv, W, K, z)
    right = _tolerances(lc.judge_rows(oracle, case, values_of, o32, rows, H, Hkv, W, K, sink=z))
    for family, (worst, tol) in right.items():
        assert worst <= tol < 1e-3, (what, family, worst, tol)
    skipped = set()
    with _items_of(item):
        for name in sl.WRONG:
            if not _applicable(name, case, rows, H, Hkv, W, case.D, epl, item):
                skipped.add(name)
                continue
            zw = z
            if name == FAR:
                top = lc.largest_score(case, H, Hkv) if largest is None else largest
                zw = np.full(H, top + sl.FAR_ABOVE, np.float32)
            wrong = _wrong_rows(name, case, values_of, rows, H, Hkv, W, K, zw, epl)
            res = lc.judge_rows(oracle, case, values_of, wrong, rows, H, Hkv, W, K, sink=zw)
            ratio = max(max(e) / right[fam][1] for fam, (e, _) in res.items())
            print(f"SINK LIMITS {what} | wrong model '{name}': worst error / tol {ratio:.3g} (biting fraction {f:.2f})")
            assert ratio > 1.0, (what, name, ratio)
    assert skipped == set(inapplicable), (what, "inapplicable wrong models", sorted(skipped))


# ---- the judge --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,Hkv,W,K", [(2, 2, 0, 0), (2, 2, 17, 0), (2, 2, 16, 4), (2, 1, 0, 0), (4, 2, 33, 5), (4, 2, 24, 20)])
def test_row_truth_with_sink_logits_is_the_dense_model(oracle, H, Hkv, W, K):
    """limit_cases.row_truth(..., sink=z) against sink_logits_model._evaluate on a dense case, with learned logits and with the
    -inf, -1e30 and +1e30 anchors: the float64 attention, its condition scale and the sink's share agree to float64 rounding;
    the float32 evaluation passes the dense model's own tolerance; -inf everywhere is the plain truth of the oracle's model."""
    lengths = [1, 16, 17, 18, 40, 63, 33, 21, 0]
    S, D = 64, 128
    case = lc.SparseCase(33, lengths, S, D, H=H, Hkv=Hkv, families={4: ("offset-", "late_peak")[:Hkv], 5: "early_peak"})
    kt, v = case.dense()
    rows = list(range(len(lengths)))
    lse = lc.judged_lse(case, case.rows, rows, H, Hkv, W, K)
    z = lc.learned_sparse(lse)
    want = sl.learned(case.q, kt, case.lengths, H, Hkv, W, K)
    assert np.abs(z - want).max() <= 1e-5, "learned_sparse over every row is sink_logits_model.learned"
    want_lse = sl.log_sum_exp(case.q, kt, case.lengths, H, Hkv, W, K)
    live = case.lengths > 0
    assert np.abs(lse[live] - want_lse[live]).max() <= 1e-12 * np.abs(want_lse[live]).max() and (lse[~live] == -np.inf).all()
    for zs, _ in [(z, {})] + sl.mixed(z):
        model = sl.SinkLogitsModel(case.q, kt, v, case.lengths, H, Hkv, zs, W, K)
        tol = sl.tolerance(model, sl.eval_fp32(case.q, kt, v, case.lengths, H, Hkv, zs, W, K))
        share = lc.sink_share(lse, zs)
        for b in np.nonzero(live)[0]:
            K_, V_ = case.rows(b)
            for h, (cols, m, (_, _, o)) in enumerate(lc.row_truth(oracle, case.q[b], K_, V_, H, Hkv, W, K, sink=zs)):
                assert np.abs(m.o[0] - model.o[b, cols]).max() <= 1e-12 * max(1.0, np.abs(model.o[b, cols]).max()), (b, h)
                assert abs(m.o_scale[0] - model.o_scale[b, h]) <= 1e-12 * model.o_scale[b, h], (b, h)
                assert abs(share[b, h] - model.share[b, h]) <= 1e-12, (b, h)
                assert fm.attention_error(o, m)[0] <= tol, (b, h)
                if zs[h] > 1e29:
                    assert not m.o.any() and not o.any() and m.o_scale[0] == 1.0
    b = 5
    K_, V_ = case.rows(b)
    for (_, m, _), (_, plain, _) in zip(lc.row_truth(oracle, case.q[b], K_, V_, H, Hkv, W, K, sink=sl.none(H)),
                                         lc.row_truth(oracle, case.q[b], K_, V_, H, Hkv, W, K)):
        assert np.abs(m.o - plain.o).max() <= 1e-14 and abs(m.o_scale[0] - plain.o_scale[0]) <= 1e-14
    with pytest.raises(AssertionError):
        lc.row_truth(oracle, case.q[b], K_, V_, H, Hkv, W, K, sink=z, cap=5.0)
    with pytest.raises(AssertionError):
        lc.row_truth(oracle, case.q[b], K_, V_, H, Hkv, W, K, sink=z, slopes=np.ones(H, np.float32))


# ---- the decode cases' small siblings ------------------------------------------------------------------------------------------
NO_GROUP, NO_WINDOW, ONE_LOAD, ONE_ITEM = ("logit of the K/V head", "sink dropped where a window is active", "one lane load only",
                                           "sink counted once per item")


@pytest.mark.parametrize("form,Hkv,W,K,inapplicable", [
    ("sink_logits", 2, 0, 0, (NO_GROUP, NO_WINDOW, ONE_LOAD, ONE_ITEM)), ("sink_logits_gqa", 1, 0, 0, (NO_WINDOW, ONE_LOAD, ONE_ITEM)),
    ("sink_logits_window", 2, 17, 0, (NO_GROUP, ONE_LOAD, ONE_ITEM)), ("sink_logits_sinks", 2, 16, 4, (NO_GROUP, ONE_LOAD, ONE_ITEM))])
def test_the_last_row_forms_bite(oracle, form, Hkv, W, K, inapplicable):
    """HEAD_FORMS' sink-logit cases on 64 rows of limit_cases.heads_case (rows of at most 63 tokens: one item, one lane load)"""
    case, named = lc.heads_case(128, B=64)
    _proof(oracle, case, case.rows, lc.sample_rows(case.B, named, n=24), 2, Hkv, W, K, f"B 64 {form}", inapplicable=inapplicable)


@pytest.mark.parametrize("W", [0, 8192])
def test_the_merge_case_bites(oracle, W):
    """MERGE_FORMS' sink-logit cases: one row of 16383 tokens and 32 heads in items of 128 -- 128 items, the sink counted once.
    Judged on four heads (0, 1, 30, 31): the wrong models are evaluated on those heads' columns as a problem of four heads with
    their four logits, so "the neighbouring head" reads another judged head's logit."""
    full = lc.merge_case((16383,))
    heads = (0, 1, 30, 31)
    hd = full.D // 32
    cols = np.concatenate([np.arange(h * hd, (h + 1) * hd) for h in heads])
    Kf, Vf = full.rows(0)
    held = (np.ascontiguousarray(Kf[:, cols]), np.ascontiguousarray(Vf[:, cols]))
    sub = SimpleNamespace(q=np.ascontiguousarray(full.q[:, cols]), lengths=full.lengths, B=1, D=len(cols), H=4,
                          family=lambda b, h=0: full.family(b, heads[h]))
    lse_full = lc.judged_lse(full, full.rows, [0], 32, 32, W, 0)
    lse_sub = lc.judged_lse(sub, lambda b: held, [0], 4, 4, W, 0)
    assert np.array_equal(lse_sub[0], lse_full[0, list(heads)]), "the four heads of the sub-problem are the case's"
    top = max(float(np.abs(held[0][:, i * hd:(i + 1) * hd] @ sub.q[0, i * hd:(i + 1) * hd].astype(np.float64)).max()) / np.sqrt(hd)
              for i in range(4))
    _proof(oracle, sub, lambda b: held, [0], 4, 4, W, 0, f"one row of 16383, 32 heads, W {W}", epl=8, item=128,
           inapplicable=(NO_GROUP, ONE_LOAD) + ((NO_WINDOW,) if W == 0 else ()), largest=top)


@pytest.mark.parametrize("elem,D,H", [("f32", 512, 4), ("bf16", 1024, 8)])
def test_the_widest_rows_bite(oracle, elem, D, H):
    """HEADS_WIDE's sink-logit cases: head size 128, two lane loads -- "one lane load only" applies"""
    case = lc.wide_case(D, flat=True)
    vals = {b: tuple(sl.rounded(a, elem) for a in case.rows(b)) for b in range(case.B)}
    _proof(oracle, case, vals.__getitem__, list(range(case.B)), H, H, 0, 0, f"widest rows D {D} {elem}", epl=lc.EPL[elem],
           inapplicable=(NO_GROUP, NO_WINDOW))


@pytest.mark.parametrize("W,K", [(63, 0), (0, 0), (59, 4)])
def test_the_window_hand_off_bites(oracle, W, K):
    """BIASED_WINDOW_CALLS' sink-logit cases on (12, 64, 128): W 63 and K 4 + W 59 (no row is longer than the window: the
    window drops nothing from a row of 63 tokens under W 63, so "dropped where a window is active" cannot show at W 63) and
    the plain mask the hand-offs W 64 and K 4 + W 60 run"""
    case = lc.window_case(128, flat=True)
    skip = (NO_GROUP, ONE_LOAD, ONE_ITEM) + ((NO_WINDOW,) if W in (0, 63) else ())
    _proof(oracle, case, case.rows, list(range(case.B)), 2, 2, W, K, f"window hand-off W {W} K {K}", inapplicable=skip)


@pytest.mark.parametrize("pair", lc.SINK_FAMILY_PAIRS)
def test_the_score_families_bite(oracle, pair):
    """The score families against the sink on ten rows of limit_cases.sink_family_case: 8 heads on 2 K/V heads, rows of up to
    1023 tokens in items of 64 -- 16 items, the sink counted once"""
    case = lc.sink_family_case(pair, B=10)
    rows = list(range(case.B))
    _proof(oracle, case, case.rows, rows, 8, 2, 0, 0, f"score families {pair}", epl=8, item=64, inapplicable=(NO_WINDOW, ONE_LOAD))
    # z = 0 for every head, the "off-by-one" softmax: what the GPU test asserts of the offset heads holds for the model
    if "offset+" in pair:
        zero = np.zeros(8, np.float32)
        for b in rows:
            if case.lengths[b]:
                Kb, Vb = case.rows(b)
                truth = lc.row_truth(oracle, case.q[b], Kb, Vb, 8, 2, sink=zero)
                plain = lc.row_truth(oracle, case.q[b], Kb, Vb, 8, 2, sink=sl.none(8))
                for h in range(8):
                    if case.family(b, h) == "offset+":
                        assert np.array_equal(truth[h][2][2], plain[h][2][2]), "expf(-200) is 0: the float32 evaluation's bits"
                    else:
                        assert np.abs(truth[h][1].o).max() <= np.exp(-150.0) * np.abs(Vb).max()


# ---- the prompt scan at 4096 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,K", [(0, 0), (1000, 20), (16, 0), (4095, 0)])
def test_the_long_prompt_comparison_bites(oracle, mli, W, K):
    """tests/test_prompt_long_gpu.py's sink-logit test on the CPU at D 64 with four heads on two K/V heads: the segments the GPU
    test keeps, logits per head from the judged queries at positions >= 1000; the float32 evaluation passes, the wrong models
    are rejected, the condition holds over the queries that set the logits."""
    seed, D, H, Hkv = 712, 64, 4, 2
    tq = mli.mli_prompt_scan_tq(D, H, 0)
    case = pm.long_case(seed, D, H, Hkv, tq, families=pm.long_sink_families(Hkv))
    segs = pm.long_reaching_segments(tq)
    rows, pos = pm.queries(segs)
    qv = pm.query_vectors(case.q, rows, pos)
    late = np.nonzero(pos >= 1000)[0]
    lse = lc.judged_lse(case, case.rows, rows[late], H, Hkv, W, K, q=qv[late], lengths=pos[late] + 1)
    z = lc.learned_sparse(lse)
    what = f"long prompt D{D} H{H}/{Hkv} W{W} K{K}"
    f = lc.biting(lse, z, what)
    truth = pm.long_truth(oracle, case, case.rows, qv, rows, pos, H, Hkv, W, K, sink=z)
    o32 = np.zeros((len(rows), D), np.float32)
    for i, heads in enumerate(truth):
        for cols, _, o, _ in heads:
            o32[i, cols] = o[0]
    res = pm.long_compare(o32, truth, what=what + " float32", report=lambda *_: None)
    pm.hm.assert_within(res, what)
    tol = {family: t for family, _, t in res}
    top = max(float(np.abs(case.rows(int(b))[0][:t + 1, (h // 2) * 16:(h // 2 + 1) * 16] @ qv[i, h * 16:(h + 1) * 16].astype(np.float64)).max()) / 4.0
              for i, (b, t) in enumerate(zip(rows, pos)) for h in range(H))
    skipped = set()
    # every early query, every fourth late one, the query at n_sequence - 1
    some = np.unique(np.concatenate([np.nonzero(pos < 1000)[0], late[::4], np.nonzero(pos == pm.LONG_S - 1)[0]]))
    for name in sl.WRONG:
        applies = {"sink dropped where a window is active": W > 0, "one lane load only": False,
                   "sink counted once per item": W == 0 or W > sl.ITEM_TOKENS}.get(name, True)
        if not applies:
            skipped.add(name)
            continue
        zw, ref = z, truth
        if name == FAR:
            zw = np.full(H, top + sl.FAR_ABOVE, np.float32)
            ref = pm.long_truth(oracle, case, case.rows, qv, rows, pos, H, Hkv, W, K, sink=zw)
        worst = 0.0
        for i in some:
            Kb, Vb = case.rows(int(rows[i]))
            t = int(pos[i])
            wrong = sl.wrong(name, qv[i][None], np.ascontiguousarray(Kb[:t + 1].T)[None], Vb[None, :t + 1], [t + 1], H, Hkv, zw, W, K)[0]
            for cols, model, _, family in ref[i]:
                worst = max(worst, float(fm.attention_error(wrong[cols][None], model)[0]) / tol[family])
        print(f"SINK LIMITS {what} | wrong model '{name}': worst error / tol {worst:.3g} (biting fraction {f:.2f})")
        assert worst > 1.0, (what, name, worst)
    assert skipped == ({"one lane load only"} | ({"sink dropped where a window is active"} if W == 0 else set())
                       | ({"sink counted once per item"} if W == 16 else set()))
