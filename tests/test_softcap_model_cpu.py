"""The soft-capping test infrastructure (tests/softcap_model.py), without a GPU:
  - on inputs whose largest score is half the largest cap (softcap_model.scale_q), at caps 50, 5 and 1 and under every form
    (W, K), the float32 evaluation of the right model stays inside the tolerance derived from it and every wrong model misses
    that tolerance by at least 4 x: the comparison the GPU tests make bites.  Two of the wrong models ARE the right model at
    cap 1 (cap * tanh(x) and tanh(x / cap)): there the test holds that they are, bit for bit, instead of asking for a margin
    that cannot exist;
  - a masked slot admitted at -cap weighs e^(-cap - max) and is invisible at cap 50 unless the live scores are that low
    themselves: that wrong model is judged on softcap_model.repelled_case;
  - the prompt form is the decode model on virtual rows;
  - the replay audit with the cap accepts a stream decoded on its own forward and rejects one decoded without the cap and one
    decoded with another cap; the engine tests' cap changes the tokens of the engine tests' model."""
import numpy as np
import pytest

import heads_model as hm
import softcap_model as sc
from helpers import paged_case

MARGIN = 4.0
LENGTHS = [2, 17, 40, 64, 100, 128]
IDENTICAL_AT_CAP_1 = ("cap * tanh(x) without the division", "tanh(x / cap) without the multiplication")


def _case(seed, B, S, D, lengths):
    c = paged_case(seed, B, S, D, conditioned=True, lengths=np.asarray(lengths, np.int32))
    return c["q_output"], c["kt_cache"], c["v_cache"], c["lengths"]


def _inputs(name):
    """(q, kt, v, L, H, Hkv, epl) on which fault `name` can show: 4 heads on 2 K/V heads at emb_dim 128; rows of two lane loads
    for the lane-load fault; scores near -2 cap for the masked-slot fault, half the largest cap at most for the others"""
    if name == "one lane load only":
        B, S, D, H, Hkv = 6, 128, 512, 8, 8
    else:
        B, S, D, H, Hkv = 6, 128, 128, 4, 2
    q, kt, v, L = _case(7300, B, S, D, LENGTHS)
    if name == "masked slots admitted at -cap":
        q, kt = sc.repelled_case(q, kt, L, H, Hkv)
    else:
        q = sc.scale_q(q, kt, L, H, Hkv)
        assert abs(sc.largest_score(q, kt, L, H, Hkv) - sc.CAPS[0] / 2) < 1e-4
    return q, kt, v, L, H, Hkv, 4


@pytest.mark.parametrize("name", sc.WRONG)
def test_every_wrong_model_misses_the_tolerance_at_every_cap_and_form(name):
    q, kt, v, L, H, Hkv, epl = _inputs(name)
    for cap in sc.CAPS:
        for W, K in sc.FORMS:
            model = sc.SoftcapModel(q, kt, v, L, H, Hkv, cap, W, K)
            o32 = sc.eval_fp32(q, kt, v, L, H, Hkv, cap, W, K)
            tol = sc.tolerance(model, o32)
            e32 = float(hm.heads_error(o32, model).max())
            bad_o = sc.wrong(name, q, kt, v, L, H, Hkv, cap, W, K, epl)
            bad = float(hm.heads_error(bad_o, model).max())
            print(f"SOFTCAP wrong model '{name}' cap {cap:g} W{W} K{K}: error {bad:.3e}, tolerance {tol:.3e} "
                  f"(float32 evaluation of the right model {e32:.3e})")
            assert e32 <= tol < 1e-4, (cap, W, K)
            if cap == 1.0 and name in IDENTICAL_AT_CAP_1:
                assert np.array_equal(bad_o, model.o), "at cap 1 this expression is the right one"
                continue
            assert bad >= MARGIN * tol, (name, cap, W, K)


def test_the_lane_load_fault_needs_rows_of_two_lane_loads():
    assert not any(sc.second_lane_load(h, 4, 128, 4) for h in range(4))
    assert [sc.second_lane_load(h, 8, 512, 4) for h in range(8)] == [False] * 4 + [True] * 4
    assert [sc.second_lane_load(h, 16, 1024, 8) for h in range(16)] == [False] * 8 + [True] * 8


def test_rows_of_one_token_and_empty_rows():
    q, kt, v, L = _case(7301, 4, 64, 128, [0, 1, 1, 30])
    q = sc.scale_q(q, kt, L, 4, 2)
    for cap in sc.CAPS:
        m = sc.SoftcapModel(q, kt, v, L, 4, 2, cap)
        assert (m.o[0] == 0).all()
        for b in (1, 2):
            for h in range(4):
                assert np.array_equal(m.o[b, hm.head_slice(h, 4, 128)], v[b, 0, hm.head_slice(h // 2, 4, 128)].astype(np.float64))


@pytest.mark.parametrize("W,K", [(0, 0), (40, 4)])
def test_the_prompt_form_is_the_decode_model_on_virtual_rows(W, K):
    import prompt_model as pm
    q, kt, v, L = _case(7302, 3, 64, 128, [64, 40, 20])
    segs = [(0, 0, 5), (1, 30, 10), (0, 60, 4), (2, 19, 1)]
    rows, pos = pm.queries(segs)
    qv = sc.scale_q(pm.query_vectors(q, rows, pos), kt[rows], pos + 1, 4, 2)
    got = sc.prompt_model(qv, kt, v, rows, pos, 4, 2, 5.0, W, K)
    for i, (b, t) in enumerate(zip(rows, pos)):
        one = sc.SoftcapModel(qv[i:i + 1], kt[b:b + 1], v[b:b + 1], [t + 1], 4, 2, 5.0, W, K)
        assert np.array_equal(one.o[0], got.o[i]), (i, b, t)
    o32 = sc.prompt_eval_fp32(qv, kt, v, rows, pos, 4, 2, 5.0, W, K)
    assert float(hm.heads_error(o32, got).max()) <= sc.tolerance(got, o32)


def test_the_audit_with_the_cap_accepts_its_own_stream_and_rejects_the_others():
    from engine_sim import make_items, make_model
    S, D, V, H = 64, 128, 1024, 4
    model, items = make_model(8648, V, S, D), make_items(9648, 6, 3, 20)
    spec = sc.SoftcapSpec("f32", H, None, 0, False, sc.ENGINE_CAP)
    right = [(i, sc.generate(model, p, spec, S)) for i, p in items]
    sc.audit(model, items, right, spec, S, what="the capped forward's own stream").assert_ok()
    for what, cap in (("without the cap", 0.0), ("with another cap", 4.0 * sc.ENGINE_CAP)):
        other = [(i, sc.generate(model, p, spec, S, wrong_cap=cap)) for i, p in items]
        assert any(len(a) != len(b) or (a != b).any() for (_, a), (_, b) in zip(right, other)), f"decoding {what} changes no token"
        fig = sc.audit(model, items, other, spec, S, what=f"a stream decoded {what}")
        assert fig.failures and not fig.bookkeeping
        assert fig.worst_ratio >= MARGIN, fig.line()


@pytest.mark.parametrize("Hkv,store", [(4, "f32"), (2, "f32"), (4, "bf16"), (2, "bf16")])
def test_the_engine_tests_cap_changes_the_tokens_of_their_model(Hkv, store):
    """tests/test_softcap_engine_gpu.py's model, items and cap: the capped CPU generator and the plain one disagree"""
    import gqa_model as gm
    from engine_sim import make_items, make_model
    S, D, V, H = 64, 128, 1024, 4
    model, items = gm.expand_model(make_model(8648, V, S, D), H, Hkv), make_items(9648, 16, 3, 20)
    capped = sc.SoftcapSpec(store, H, None, 0, False, sc.ENGINE_CAP)
    differ = sum(len(a) != len(b) or (a != b).any()
                 for a, b in ((sc.generate(model, p, capped, S), sc.generate(model, p, capped, S, wrong_cap=0.0)) for _, p in items))
    assert differ >= len(items) // 2, differ
