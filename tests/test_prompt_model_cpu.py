"""Proves on the CPU that the comparisons of tests/test_prompt_scan_gpu.py and tests/test_prompt_logprobs_engine_gpu.py bite
(tests/prompt_model.py).

The scan: at the shapes, forms and segment lists of the GPU test the model on the virtual rows (query t = the decode problem of
a row of length t + 1: gqa_model / sinks_model / window_model / heads_model) agrees row by row with the scan stated directly,
the fp32 oracle passes against it with its own tolerance, and six wrong scans fail the same comparer at the same tolerance: the
query attends slot t + 1; the window's lower bound off by one at either end; sinks dropped; K/V head h instead of h / g; the
second segment of a row scored with its positions restarted at 0.

The figures: on an engine_sim model the prompt figures of logprobs_model.reference with the target shifted by one are rejected
at the bound the engine test uses."""
import functools

import numpy as np
import pytest

import gqa_model as gm
import heads_model as hm
import prompt_model as pm
import replay_model as rm
from accuracy_cases import apply_family, base_case

ELEM = {"f32": 0, "bf16": 1}
CPU_SHAPES = [s for s in pm.SHAPES if s[1] <= 512]


@functools.lru_cache(maxsize=4)
def _case(seed, D, tq):
    segs, lengths = pm.segments_for(tq)
    return segs, lengths, base_case(seed, len(lengths), pm.S, D, lengths)


def _operands(c, H, Hkv, assignment):
    if H == 1:
        q, kt = apply_family(c, assignment)
        return q, kt, (assignment,)
    q, kt = gm.apply_gqa_families(c, H, Hkv, assignment)
    return q, kt, gm.head_families(assignment, H, Hkv)


@pytest.mark.parametrize("W,K", pm.FORMS)
@pytest.mark.parametrize("seed,D,H,Hkv,elem", CPU_SHAPES)
def test_virtual_rows_are_the_scan_and_wrong_scans_fail(oracle, mli, seed, D, H, Hkv, elem, W, K):
    tq = mli.mli_prompt_scan_tq(D, H, ELEM[elem])
    assert tq in (2, 4, 8)
    segs, lengths, c = _case(seed, D, tq)
    rows, pos = pm.queries(segs)
    assert pos.max() == pm.S - 1 and {0, 15, 16, 17} <= {f for _, f, _ in segs}
    assert {1, tq - 1, tq, tq + 1, 2 * tq + 1} - {0} <= {n for _, _, n in segs}
    assert len({r for r, _, _ in segs}) < len(segs) and [r for r, _, _ in segs] != sorted(r for r, _, _ in segs)
    for assignment in (("flat", "offset-") if H == 1 else ("flat", "mixed")):
        q, kt, fams = _operands(c, H, Hkv, assignment)
        v = c["v_cache"]
        qv = pm.query_vectors(q, rows, pos)
        model = pm.model_prompt(qv, kt, v, rows, pos, H, Hkv, W, K)
        direct = pm.scan_float64(qv, kt, v, rows, pos, H, Hkv, W, K)
        assert np.abs(model.o - direct).max() <= 1e-12 * max(1.0, np.abs(direct).max()), "query t is the row of length t + 1"
        o_or = pm.oracle_prompt(oracle, qv, kt, v, rows, pos, H, Hkv, W, K)
        what = f"D{D} H{H}/{Hkv} W{W} K{K} {assignment}"
        gm.assert_within(gm.compare(o_or, o_or, model, fams, what=what + " oracle", report=lambda *_: None), what)
        if assignment != "flat":
            continue
        for name in pm.SCAN_MUTANTS:
            wrong, applies = pm.scan_mutant(name, segs, lengths, qv, kt, v, rows, pos, H, Hkv, W, K)
            res = gm.compare(wrong, o_or, model, fams, what=f"{what} {name}", report=lambda *_: None)
            ratio = max(worst / tol for _, worst, tol in res)
            if applies:
                assert ratio > 1.0, (what, name, ratio)
            else:
                assert ratio <= 1.0, (what, name, ratio)


def test_every_variant_and_every_form_is_covered(mli):
    variants = set()
    for _, D, H, Hkv, elem in pm.SHAPES:
        epl = 4 if elem == "f32" else 8
        variants.add((elem, -(-(D // epl) // 64), H > 1))
        assert mli.mli_prompt_scan_tq(D, H, ELEM[elem]) >= 2
    assert variants == {(e, nj, h) for e in ("f32", "bf16") for nj in (1, 2) for h in (False, True)}
    assert any(D // (4 * 64) == 0 and D % 256 for _, D, H, _, e in pm.SHAPES if e == "f32"), "a partly filled lane load"
    assert {(8, 2), (8, 1)} <= {(H, Hkv) for _, _, H, Hkv, _ in pm.SHAPES}
    assert {D // H for _, D, H, _, _ in pm.SHAPES if H == 4} >= {32, 64}
    assert set(pm.FORMS) == {(0, 0), (40, 0), (40, 4), (16, 0)}


@pytest.mark.parametrize("kind,n_heads,window,sinks", [("PAGED", 1, None, 0), ("PAGED_BF16", 4, 40, 4)])
def test_a_target_shifted_by_one_is_rejected(kind, n_heads, window, sinks):
    model, items, _ = rm.sampled_workload("top-p")
    spec = rm.spec_of_kind(kind, n_heads, window, sinks, native=False)
    n_top = 3
    rejected = 0
    for item_id, prompt in items[:6]:
        toks = np.concatenate([np.asarray(prompt, np.int32), [7, 9]])          # any continuation: the prompt rows do not see it
        rep = pm.prompt_replay(model, toks, len(prompt), spec)
        bound, e32 = pm.prompt_bound(rep)
        assert len(rep.rows) == len(prompt) - 1 and bound > 0 and e32 < bound
        right = pm.prompt_reference(rep.logits, toks, n_top)
        # the float32 restatement of the forward, scored in float64, passes its own bound
        lg32 = rep.logits32()
        m = lg32.max(axis=1, keepdims=True)
        lp32 = lg32 - m - np.log(np.exp(lg32 - m).sum(axis=1, keepdims=True))
        given = pm.prompt_targets(toks, len(lg32))
        assert np.abs(lp32[np.arange(len(given)), given] - right[0]).max() <= bound
        for shift in (0, 2):
            wrong = pm.prompt_reference(rep.logits, toks, n_top, shift=shift)
            rejected += bool(np.abs(wrong[0] - right[0]).max() > bound)
    assert rejected == 12, rejected


def test_given_reference_reports_alternatives_for_a_token_out_of_range():
    x = np.asarray([[0.0, 1.0, 2.0, -np.inf], [-np.inf] * 4], np.float32)
    lp, ids, lps = pm.given_reference(x, [7, 1], 2)
    assert lp[0] == -np.inf and ids[0].tolist() == [2, 1] and np.isfinite(lps[0]).all()
    assert lp[1] == -np.inf and ids[1].tolist() == [-1, -1]
    lp, _, _ = pm.given_reference(x, [2, -1], 0)
    assert np.isclose(lp[0], 2.0 - np.log(np.exp(0.0) + np.exp(1.0) + np.exp(2.0)))
