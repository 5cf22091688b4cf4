"""mli_prompt_scan_paged_mfma held to fp32 rounding error against the float64 model on the virtual rows
(tests/prompt_model.py), on the rounded bf16 pool.  n_sequence 128; (D, H, Hkv): (256, 4, 4) g 1 hd 64 | (512, 8, 2) g 4 hd 64, four
column tiles | (512, 4, 1) g 4 hd 128 | (1024, 8, 1) g 8 hd 128 | (2048, 16, 4), which no other prompt scan takes -- each plain, under
window 40 and under window 16.  Segments: prompt_model.segments_for by the shape's mli_prompt_scan_mfma_tq.
Tolerance: f64_model.tolerance of the fp32 CPU oracle's own error on the same virtual rows, per score family; one bf16 part of q
and of the probabilities must EXCEED it on the same inputs (numpy), so the comparison bites.  NaN in every K / V slot above a row's
last scored position, below the window of every query of the row, in the K / V columns >= Hkv * hd, in the pages beyond a row's last
page and in the q rows of no query; `out` rows of no query keep their sentinel; within twice the bound of mli_prompt_scan_paged where
that kernel takes the shape; one "scan_prompt_mfma" launch and no other scan family."""
import functools

import numpy as np
import pytest
import torch

import f64_model as fm
import gqa_model as gm
import heads_model as hm
import prompt_model as pm
from accuracy_cases import base_case, fill_pages
from gpu_util import host
from test_gqa_mfma_scan_gpu import _one_part_model
from test_gqa_scan_gpu import _unread_offsets
from test_prompt_scan_gpu import HOLE, HOLE_AFTER, TAIL, _distance
from test_window_scan_gpu import ELEM, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

SHAPES = [(721, 256, 4, 4), (722, 512, 8, 2), (723, 512, 4, 1), (724, 1024, 8, 1), (725, 2048, 16, 4)]
WINDOWS = (0, 40, 16)


@functools.lru_cache(maxsize=2)
def _case(seed, D, tq):
    segs, lengths = pm.segments_for(tq)
    return segs, lengths, base_case(seed, len(lengths), pm.S, D, lengths)


def _below_window_offsets(c, segs, D, W):
    """Pool offsets of the K and V slots below the window of EVERY query of their row"""
    lo = {}
    for r, f, _ in segs:
        lo[r] = min(lo.get(r, pm.S), max(0, f + 1 - W))
    out = [np.zeros(0, np.int64)]
    for r, top in lo.items():
        s = np.arange(top if W else 0)
        slot = c["table"][r, s // 16].astype(np.int64) + (s % 16) * 3 * D
        out.append((slot[:, None] + np.concatenate([D + np.arange(D), 2 * D + np.arange(D)])[None, :]).reshape(-1))
    return np.concatenate(out)


@pytest.mark.parametrize("W", WINDOWS)
@pytest.mark.parametrize("seed,D,H,Hkv", SHAPES)
def test_prompt_mfma_scan(oracle, mli, dev, seed, D, H, Hkv, W):
    from min_llm_inference_amd import ops
    S, bf16 = pm.S, ELEM["bf16"]
    assert mli.mli_prompt_scan_mfma_shape_supported(9, S, D, H, Hkv, bf16) == 1
    tq = ops.prompt_scan_mfma_tq(D, H, Hkv)
    segs, lengths, c = _case(seed, D, tq)
    rows, pos = pm.queries(segs)
    counts = [cnt for _, _, cnt in segs]
    dense = np.concatenate([[0], np.cumsum(counts)[:-1]])
    offsets = dense + np.where(np.arange(len(segs)) > HOLE_AFTER, HOLE, 0)
    where = np.concatenate([np.arange(o, o + cnt) for o, cnt in zip(offsets, counts)])     # the out row of every query
    n_rows = len(rows) + HOLE + TAIL
    nobody = np.setdiff1d(np.arange(n_rows), where)
    seg_arrays = tuple(_t(np.asarray(a, np.int32), dev) for a in (*zip(*segs), offsets)) + (max(counts),)
    nan_page = _nan_page(D, "bf16", dev)
    others = [f for f in ops.launch_families() if f.startswith("scan_") and f != "scan_prompt_mfma"]
    results = []
    for assignment in hm.ASSIGNMENTS:
        what = f"MFMA D{D} H{H}/{Hkv} W{W} TQ{tq} {assignment}"
        q, kt = gm.apply_gqa_families(c, H, Hkv, assignment)
        fams = gm.head_families(assignment, H, Hkv)
        pool32, off = fill_pages(oracle, c, q, kt, c["v_cache"])
        poison = np.concatenate([off, _below_window_offsets(c, segs, D, W), _unread_offsets(c, D, Hkv * (D // H))])
        pool, values = _poisoned_pool(pool32, poison, "bf16", dev)
        ktm = fm.gather_pages(values, c["table"], lengths, S, D, 1).transpose(0, 2, 1)
        v_rows = fm.gather_pages(values, c["table"], lengths, S, D, 2)
        table = _t(np.where(c["table"] >= 0, pool.data_ptr() + 2 * c["table"], nan_page.data_ptr()).astype(np.int64), dev)
        qv = pm.query_vectors(q, rows, pos)
        model = pm.model_prompt(qv, ktm, v_rows, rows, pos, H, Hkv, W, 0)
        o_or = pm.oracle_prompt(oracle, qv, ktm, v_rows, rows, pos, H, Hkv, W, 0)
        q_dev = torch.full((n_rows, D), float("nan"), device=dev)
        q_dev[_t(where, dev)] = _t(qv, dev)
        out = torch.full((n_rows, D), SENTINEL, device=dev)
        ops.reset_launch_counts()
        ops.prompt_scan_paged(q_dev, table, None, out, len(lengths), S, bf16, n_heads=H, n_kv_heads=Hkv, window=W,
                              seg_arrays=seg_arrays, mfma=True)
        assert ops.launch_count("scan_prompt_mfma") == 1 and not any(ops.launch_count(f) for f in others), what
        got_all = host(out).copy()
        assert (got_all[nobody] == SENTINEL).all(), f"{what}: an out row of no query was written"
        got = got_all[where]
        assert np.isfinite(got).all() and (got != SENTINEL).any(axis=1).all(), what
        res = gm.compare(got, o_or, model, fams, what=what)      # prints worst error and tolerance per family
        results += res
        if D <= 1024:                     # mli_prompt_scan_paged takes bf16 rows of at most two lane loads
            ref = torch.full((n_rows, D), SENTINEL, device=dev)
            ops.prompt_scan_paged(q_dev, table, None, ref, len(lengths), S, bf16, n_heads=H, n_kv_heads=Hkv, window=W,
                                  seg_arrays=seg_arrays)
            d = _distance(got, host(ref)[where], model)
            for family, _, tol in res:
                worst = float(d[:, [h for h in range(H) if fams[h] == family]].max())
                print(f"{what} | {family}: {worst:.3e} from mli_prompt_scan_paged, twice the bound {2 * tol:.3e}")
                assert worst <= 2 * tol, (what, family, worst, tol)
        if W == 0 and assignment == hm.ASSIGNMENTS[0]:
            ktv, vv, Lv = pm.virtual(ktm, v_rows, rows, pos)
            rounded = gm.compare(_one_part_model(qv, ktv, vv, Lv, H, Hkv), o_or, model, fams, what="one bf16 part",
                                 report=lambda s: None)
            assert any(worst > tol for _, worst, tol in rounded), "one bf16 part of q and of the probabilities stays inside the bound"
    gm.assert_within(results, f"MFMA D{D} H{H}/{Hkv} W{W}")
