"""Proves on the CPU that the comparison of tests/test_prompt_long_gpu.py bites at n_sequence 4096 (tests/prompt_model.py, the
long-prompt part): on the segments of the GPU test, form by form, the judge passes the fp32 oracle, rejects the six
prompt_model.SCAN_MUTANTS, and rejects three wrong scans that only long rows can show -- every fourth page from the fifth on
skipped (a wave that loses its stride), the sink run one page short, the dropped run one page too long.  Every mutant must be
rejected in every form where it changes the slots some query attends, and must apply in some form.

Two shapes, so that the CPU suite stays quick: one head at D 64 (prompt_model.SHAPES[0]) and four heads on two K/V heads at D 64 (the
grouping mutant needs grouped heads); a mutant is evaluated on the queries whose attended slots it changes."""
import functools

import numpy as np
import pytest

import f64_model as fm
import prompt_model as pm

ELEM = {"f32": 0, "bf16": 1}
CPU_SHAPES = [pm.SHAPES[0], (712, 64, 4, 2, "f32")]
MUTANTS = tuple(pm.SCAN_MUTANTS) + tuple(pm.LONG_MUTANTS)


@functools.lru_cache(maxsize=1)
def _case(seed, D, H, Hkv, tq):
    return pm.long_case(seed, D, H, Hkv, tq)


def test_the_long_segments_are_what_the_issue_names(mli):
    S = pm.LONG_S
    for tq in (2, 4, 8):
        lengths = pm.long_lengths(tq)
        for W, K in pm.LONG_FORMS:
            segs = pm.long_segments(tq, W)
            rows, pos = pm.queries(segs)
            assert pos.max() == S - 1 and (lengths[rows] > pos).all()
            assert (0, S - (3 * tq + 1), 3 * tq + 1) in segs and (3, 2047 - tq, 2 * tq + 1) in segs
            assert (1, 16 * pm.LONG_K - 1, tq + 1) in segs and (5, 1000, 4 * 16 + 3) in segs and (2, 0, 1) in segs
            assert max(n for _, _, n in segs) == 4 * 16 + 3
            assert [f for r, f, _ in segs if r == 6][1] == 3000, "a continuation pass"
            assert [r for r, _, _ in segs] != sorted(r for r, _, _ in segs), "rows in permuted order"
            if 0 < W <= 1000:
                starts = {(f + 1 - W) % 16 for r, f, _ in segs if r in (4, 7)}
                assert starts == {0, 15}, "a window that starts on a page edge and one that starts at slot 15"
    assert set(pm.LONG_FORMS) == {(0, 0), (1000, 0), (1000, 20), (1000, 16), (16, 0), (24, 40), (4095, 0), (4096, 0)}
    # what the forms reach, by the arithmetic of prompt_scan_body.hpp for the block of the last query
    t0 = S - 1
    for W, K in pm.LONG_FORMS:
        p_lo = max(0, t0 + 1 - W) // 16 if W else 0
        ps = min(-(-K // 16), p_lo)
        skip = p_lo - ps
        if (W, K) in ((1000, 0), (1000, 20), (1000, 16)):
            assert skip >= 190 - 5 and ps == -(-K // 16)
        if (W, K) == (1000, 20):
            assert ps == 2 and K % 16 != 0
        if (W, K) == (4095, 0):
            assert skip == 0 and max(0, t0 + 1 - W) == 1


@pytest.mark.parametrize("seed,D,H,Hkv,elem", CPU_SHAPES)
def test_the_judge_passes_the_oracle_and_rejects_the_mutants(oracle, mli, seed, D, H, Hkv, elem):
    """Form by form: the oracle passes; every mutant that changes the slots some query attends is rejected.  Over the forms of
    one shape every mutant applies somewhere (the grouping mutant with grouped heads only): one that applied in no form would
    be an error of the test."""
    tq = mli.mli_prompt_scan_tq(D, H, ELEM[elem])
    case = _case(seed, D, H, Hkv, tq)
    applied_somewhere = {name: False for name in MUTANTS}
    truths = {}
    for W, K in pm.LONG_FORMS:
        segs = pm.long_segments(tq, W)
        rows, pos = pm.queries(segs)
        qv = pm.query_vectors(case.q, rows, pos)
        truth = pm.long_truth(oracle, case, case.rows, qv, rows, pos, H, Hkv, W, K, cache=truths)
        what = f"D{D} H{H}/{Hkv} W{W} K{K}"
        o_or = np.zeros((len(rows), D), np.float32)
        for i, heads in enumerate(truth):
            for cols, _, o, _ in heads:
                o_or[i, cols] = o[0]
        res = pm.long_compare(o_or, truth, what=what + " oracle", report=lambda *_: None)
        pm.hm.assert_within(res, what)
        tol = {family: t for family, _, t in res}
        for name in MUTANTS:
            worst, applied = 0.0, False
            for i in range(len(rows)):
                Kb, Vb = case.rows(int(rows[i]))
                wrong, applies = pm.long_mutant(name, segs, case.lengths, qv[i], Kb, Vb, i, pos, H, Hkv, W, K)
                if not applies:
                    continue
                applied = True
                for cols, model, _, family in truth[i]:
                    worst = max(worst, float(fm.attention_error(wrong[cols][None], model)[0]) / tol[family])
            applied_somewhere[name] = applied_somewhere[name] or applied
            if applied:
                assert worst > 1.0, (what, name, worst)
    never = [n for n, a in applied_somewhere.items() if not a and (Hkv < H or "K/V head" not in n)]
    assert not never, f"mutants that applied in no form: {never}"
