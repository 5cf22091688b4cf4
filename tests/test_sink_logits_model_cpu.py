"""The sink-logit test infrastructure (tests/sink_logits_model.py), without a GPU:
  - the model against a direct concatenate-and-drop float64 softmax, softmax([x, z])[:-1] . V, and against the model WITHOUT a
    sink on the row lengthened by one attended token of zero V and score z_h;
  - all logits -inf: gqa_model.model_gqa; -1e30: that model in the head's columns; +1e30: exact zeros, nothing non-finite;
  - on the inputs the GPU tests use (sink_logits_model.SCAN_CASES, every form) the float32 evaluation of the right model stays
    inside the tolerance derived from it, the condition on the logits holds (sink_logits_model.conditioned), and every wrong
    model misses that tolerance by at least 4 x where its fault can show: the comparison the GPU tests make bites;
  - the prompt form is the decode model on virtual rows;
  - the replay audit with the sink accepts a stream decoded on its own forward and rejects one decoded without the sink; the
    engine tests' logits change the tokens of the engine tests' model."""
import math

import numpy as np
import pytest

import gqa_model as gm
import heads_model as hm
import sink_logits_model as sl
from helpers import paged_case

MARGIN = 4.0
LENGTHS = [0, 1, 2, 17, 40, 64, 100, 128]


def _case(seed, B, S, D, lengths):
    c = paged_case(seed, B, S, D, conditioned=True, lengths=np.asarray(lengths, np.int32))
    return c["q_output"], c["kt_cache"], c["v_cache"], c["lengths"]


@pytest.mark.parametrize("H,Hkv", [(4, 4), (4, 2), (4, 1)])
@pytest.mark.parametrize("W,K", sl.FORMS)
def test_the_model_is_a_softmax_with_one_more_logit_whose_mass_is_dropped(H, Hkv, W, K):
    q, kt, v, L = _case(7400, 8, 128, 128, LENGTHS)
    z = sl.learned(q, kt, L, H, Hkv, W, K)
    model = sl.SinkLogitsModel(q, kt, v, L, H, Hkv, z, W, K)
    mask = sl.attended(L, 128, W, K)
    D, g, hd = 128, H // Hkv, 128 // H
    for b in range(8):
        for h in range(H):
            qs, ks = hm.head_slice(h, H, D), hm.head_slice(h // g, H, D)
            if L[b] == 0:
                assert (model.o[b, qs] == 0).all()
                continue
            s = np.nonzero(mask[b])[0]
            x = (q[b, qs].astype(np.float64) @ kt[b, ks][:, s].astype(np.float64)) / math.sqrt(hd)
            both = np.concatenate([x, [np.float64(z[h])]])
            p = np.exp(both - both.max())
            p /= p.sum()
            want = p[:-1] @ v[b, s][:, ks].astype(np.float64)
            assert np.abs(model.o[b, qs] - want).max() <= 1e-13 * max(1.0, np.abs(want).max()), (b, h)
            assert abs(model.share[b, h] - p[-1]) <= 1e-13


@pytest.mark.parametrize("H", [2, 4])
def test_the_model_equals_the_plain_model_with_an_extra_token_of_zero_v_and_score_z(H):
    """the plain form without grouping: the row lengthened by sink_logits_model.crafted_token"""
    q, kt, v, L = _case(7401, 8, 128, 128, [0, 1, 2, 17, 40, 64, 100, 127])
    z = sl.learned(q, kt, L, H, H)
    k_row, v_row = sl.crafted_token(q, H, H, z)
    kt2, v2 = kt.copy(), v.copy()
    for b in range(8):
        kt2[b, :, L[b]] = k_row[b]
        v2[b, L[b]] = v_row[b]
    longer = gm.model_gqa(q.astype(np.float64), kt2.astype(np.float64), v2.astype(np.float64), L + 1, H, H)
    model = sl.SinkLogitsModel(q, kt, v, L, H, H, z)
    live = L > 0
    # (the crafted K row is rounded to float32: its score is z_h to about 2^-24 relative, not exactly)
    assert np.abs(longer.o[live] - model.o[live]).max() <= 1e-5 * np.abs(model.o[live]).max()
    assert np.abs(longer.o[live] - gm.model_gqa(q, kt, v, L, H, H).o[live]).max() > 1e-2, "the extra token changes nothing"


@pytest.mark.parametrize("Hkv", [4, 2])
@pytest.mark.parametrize("W,K", sl.FORMS)
def test_none_is_the_gqa_model_and_the_far_logits_behave_as_stated(Hkv, W, K):
    H, D = 4, 128
    q, kt, v, L = _case(7402, 8, 128, D, LENGTHS)
    plain = gm.model_gqa(q.astype(np.float64), kt.astype(np.float64), v.astype(np.float64), L, H, Hkv, W, K)
    none = sl.SinkLogitsModel(q, kt, v, L, H, Hkv, sl.none(H), W, K)
    # (two float64 expressions of one function: equal to float64 rounding, and the condition scales likewise)
    assert np.abs(none.o - plain.o).max() <= 1e-14 * np.abs(plain.o).max()
    assert np.abs(none.o_scale - plain.o_scale)[L > 0].max() <= 1e-14 * plain.o_scale[L > 0].max()
    assert (none.share == 0).all()
    assert np.array_equal(sl.eval_fp32(q, kt, v, L, H, Hkv, sl.none(H), W, K),
                          sl.eval_fp32(q, kt, v, L, H, Hkv, np.full(H, -1e30, np.float32), W, K))
    for z, heads in sl.mixed(sl.learned(q, kt, L, H, Hkv, W, K)):
        for o in (sl.SinkLogitsModel(q, kt, v, L, H, Hkv, z, W, K).o, sl.eval_fp32(q, kt, v, L, H, Hkv, z, W, K)):
            assert np.isfinite(o).all()
            for kind in ("-inf", "-1e30"):
                sl_ = hm.head_slice(heads[kind], H, D)
                if o.dtype == np.float64:
                    assert np.array_equal(o[:, sl_], none.o[:, sl_]), kind
            assert (o[:, hm.head_slice(heads["+1e30"], H, D)] == 0).all()
            assert (o[L == 0] == 0).all()
    for z, _ in sl.mixed(np.zeros(2, np.float32)):
        assert len(z) == 2
    assert {k for _, heads in sl.mixed(np.zeros(2, np.float32)) for k in heads} == {"-inf", "-1e30", "+1e30"}


def _applies(name, H, Hkv, D, elem, S, W):
    epl = 4 if elem == "f32" else 8
    # (a window of 40 leaves one item: several items per row exist in the plain form on rows longer than an item)
    return {"logit of the K/V head": Hkv < H, "sink counted once per item": W == 0 and S > sl.ITEM_TOKENS,
            "sink dropped where a window is active": W > 0,
            "one lane load only": any(sl.second_lane_load(h, H, D, epl) for h in range(H))}.get(name, True)


@pytest.mark.parametrize("seed,B,S,D,H,Hkv,elem,chunks", sl.SCAN_CASES)
def test_on_the_gpu_tests_inputs_the_right_model_passes_and_every_wrong_one_fails(seed, B, S, D, H, Hkv, elem, chunks):
    q, kt, v, L = sl.scan_operands(seed, B, S, D, elem)
    epl = 4 if elem == "f32" else 8
    for W, K in sl.FORMS:
        z = sl.learned(q, kt, L, H, Hkv, W, K)
        model = sl.SinkLogitsModel(q, kt, v, L, H, Hkv, z, W, K)
        f = sl.conditioned(model, f"{seed} {elem} H{H}/{Hkv} W{W} K{K}")
        o32 = sl.eval_fp32(q, kt, v, L, H, Hkv, z, W, K)
        tol, e32 = sl.tolerance(model, o32), float(hm.heads_error(o32, model).max())
        assert e32 <= tol < 1e-4
        for zm, _ in sl.mixed(z):
            mm = sl.SinkLogitsModel(q, kt, v, L, H, Hkv, zm, W, K)
            om = sl.eval_fp32(q, kt, v, L, H, Hkv, zm, W, K)
            assert float(hm.heads_error(om, mm).max()) <= sl.tolerance(mm, om) < 1e-4
        for name in sl.WRONG:
            if not _applies(name, H, Hkv, D, elem, S, W):
                continue
            zw, ref = z, model
            if name == "maximum over the scores only":
                zw = np.full(H, sl.largest_score(q, kt, L, H, Hkv, W, K) + sl.FAR_ABOVE, np.float32)
                ref = sl.SinkLogitsModel(q, kt, v, L, H, Hkv, zw, W, K)
            with np.errstate(invalid="ignore"):
                bad = float(np.nan_to_num(hm.heads_error(sl.wrong(name, q, kt, v, L, H, Hkv, zw, W, K, epl), ref), nan=np.inf).max())
            print(f"SINK_LOGITS wrong model '{name}' {seed} {elem} H{H}/{Hkv} W{W} K{K}: error {bad:.3e}, tolerance {tol:.3e} "
                  f"(float32 evaluation of the right model {e32:.3e}; biting fraction {f:.2f})")
            assert bad >= MARGIN * tol, (name, W, K)


def test_the_lane_load_fault_needs_rows_of_two_lane_loads():
    assert not any(sl.second_lane_load(h, 2, 64, 4) for h in range(2))
    assert [sl.second_lane_load(h, 8, 512, 4) for h in range(8)] == [False] * 4 + [True] * 4
    assert not any(sl.second_lane_load(h, 8, 512, 8) for h in range(8))


@pytest.mark.parametrize("W,K", [(0, 0), (40, 4)])
def test_the_prompt_form_is_the_decode_model_on_virtual_rows(W, K):
    import prompt_model as pm
    q, kt, v, L = _case(7403, 3, 64, 128, [64, 40, 20])
    segs = [(0, 0, 5), (1, 30, 10), (0, 60, 4), (2, 19, 1)]
    rows, pos = pm.queries(segs)
    qv = pm.query_vectors(q, rows, pos)
    z = sl.learned(qv, kt[rows], pos + 1, 4, 2, W, K)
    got = sl.prompt_model(qv, kt, v, rows, pos, 4, 2, z, W, K)
    for i, (b, t) in enumerate(zip(rows, pos)):
        one = sl.SinkLogitsModel(qv[i:i + 1], kt[b:b + 1], v[b:b + 1], [t + 1], 4, 2, z, W, K)
        assert np.array_equal(one.o[0], got.o[i]), (i, b, t)
    o32 = sl.prompt_eval_fp32(qv, kt, v, rows, pos, 4, 2, z, W, K)
    assert float(hm.heads_error(o32, got).max()) <= sl.tolerance(got, o32)


def test_the_audit_with_the_sink_accepts_its_own_stream_and_rejects_one_without():
    from engine_sim import make_items, make_model
    S, D, V, H = 64, 128, 1024, 4
    model, items = make_model(8648, V, S, D), make_items(9648, 6, 3, 20)
    spec = sl.SinkLogitsSpec("f32", H, None, 0, False, sl.ENGINE_LOGITS)
    right = [(i, sl.generate(model, p, spec, S)) for i, p in items]
    sl.audit(model, items, right, spec, S, what="the sink forward's own stream").assert_ok()
    none = sl.SinkLogitsSpec("f32", H, None, 0, False, tuple(float(t) for t in sl.none(H)))
    plain = [(i, sl.generate(model, p, none, S)) for i, p in items]
    import replay_model as rm
    rm.audit(model, items, plain, rm.Spec("f32", H, None, 0, False), S, what="all -inf is the plain forward").assert_ok()
    other = [(i, sl.generate(model, p, spec, S, wrong_logits=())) for i, p in items]
    assert all(np.array_equal(a, b) for (_, a), (_, b) in zip(plain, other))
    assert any(len(a) != len(b) or (a != b).any() for (_, a), (_, b) in zip(right, other)), "decoding without the sink changes no token"
    fig = sl.audit(model, items, other, spec, S, what="a stream decoded without the sink")
    assert fig.failures and not fig.bookkeeping
    assert fig.worst_ratio >= MARGIN, fig.line()


@pytest.mark.parametrize("Hkv,store", [(4, "f32"), (2, "f32"), (4, "bf16"), (2, "bf16")])
def test_the_engine_tests_logits_change_the_tokens_of_their_model(Hkv, store):
    """tests/test_sink_logits_engine_gpu.py's model, items and logits: the CPU generator with the sink and the plain one disagree"""
    from engine_sim import make_items, make_model
    S, D, V, H = 64, 128, 1024, 4
    model, items = gm.expand_model(make_model(8648, V, S, D), H, Hkv), make_items(9648, 16, 3, 20)
    spec = sl.SinkLogitsSpec(store, H, None, 0, False, sl.ENGINE_LOGITS)
    differ = sum(len(a) != len(b) or (a != b).any()
                 for a, b in ((sl.generate(model, p, spec, S), sl.generate(model, p, spec, S, wrong_logits=())) for _, p in items))
    assert differ >= len(items) // 2, differ
