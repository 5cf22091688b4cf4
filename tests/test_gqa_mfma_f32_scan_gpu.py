"""mli_decode_scan_paged_gqa_mfma_f32 held to fp32 rounding error against the float64 model on the expanded operands:
tests/test_gqa_mfma_scan_gpu.py's lengths, forced item sizes, cache policies, NaN poison and tolerance (f64_model.tolerance,
unchanged) on fp32 pages.  SHAPES: hd 64, one round of K loads, plain and under a window that cuts a page | the widest row, g 4 at
hd 128, which no other fp32 scan takes | plain multi-head attention there | odd g, padded tile columns | many items, the last
arriver's merge.  On the first shape the lane-group scan runs on the same pool: the two lie within twice the bound of each other."""
import functools

import numpy as np
import pytest
import torch

import f64_model as fm
import gqa_model as gm
import sinks_model as sm
from accuracy_cases import base_case, fill_pages
from gpu_util import host
from helpers import assert_equal
from test_gqa_mfma_scan_gpu import _length_vectors
from test_gqa_scan_gpu import _device_tables, _unread_offsets
from test_window_scan_gpu import ELEM, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

SHAPES = [(901, 6, 128, 256, 4, 2, (0, 40)), (902, 5, 256, 2048, 16, 4, (0,)), (903, 5, 256, 2048, 16, 16, (0,)),
          (904, 5, 128, 448, 7, 1, (0, 17)), (905, 4, 1024, 1024, 8, 2, (0, 513))]
CASES = [(seed, B, S, D, H, Hkv, W, part, assignment) for seed, B, S, D, H, Hkv, windows in SHAPES for W in windows
         for part in range(len(_length_vectors(seed, B, S, W))) for assignment in ("mixed", "offsets")]


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, W, part):
    return base_case(seed, B, S, D, _length_vectors(seed, B, S, W)[part])


@pytest.mark.parametrize("seed,B,S,D,H,Hkv,W,part,assignment", CASES)
def test_gqa_mfma_f32_scan(oracle, mli, dev, seed, B, S, D, H, Hkv, W, part, assignment):
    from min_llm_inference_amd import ops
    assert mli.mli_gqa_mfma_f32_shape_supported(B, S, D, H, Hkv) == 1
    assert {0, 1, 16, 17, 63, 64, 65, S - 1, S} | ({W} if W else set()) <= set(_length_vectors(seed, B, S, W).reshape(-1).tolist())
    c = _base(seed, B, S, D, W, part)
    L, hd = c["lengths"], D // H
    q, kt = gm.apply_gqa_families(c, H, Hkv, assignment)
    pool32, off = fill_pages(oracle, c, q, kt, c["v_cache"])
    pages = c["table"][c["table"] >= 0].astype(np.int64)
    x_seg = (pages[:, None, None] + (np.arange(16) * 3 * D)[None, :, None] + np.arange(D)[None, None, :]).reshape(-1)
    gap = sm.gap_offsets(c["table"], L, S, D, W, 0) if W else np.zeros(0, np.int64)
    pool, values = _poisoned_pool(pool32, np.concatenate([off, gap, x_seg, _unread_offsets(c, D, Hkv * hd)]), "f32", dev)
    s_live = max(-(-int(L.max()) // 16) * 16, 16)
    ktm = fm.gather_pages(values, c["table"], L, s_live, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, s_live, D, 2)
    model, want = gm.model_gqa(q, ktm, v_rows, L, H, Hkv, W), gm.oracle_gqa(oracle, q, ktm, v_rows, L, H, Hkv, W)
    fams = gm.head_families(assignment, H, Hkv)
    _, table, _ = _device_tables(c, pool, "f32", W, 0, _nan_page(D, "f32", dev), dev)
    qd, Ld = _t(q, dev), _t(L, dev)

    def run():
        out = torch.full((B, D), SENTINEL, device=dev)
        ops.decode_scan_paged_gqa_mfma_f32(qd, table, Ld, out, H, Hkv, W, S)
        return host(out).copy()

    others = [f for f in ops.launch_families() if f.startswith("scan_") and f != "scan_gqa_mfma_f32"]
    results = []
    try:
        for ct in (64, 0):
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            what = f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} part {part} {assignment} chunk_tokens {ct}"
            ops.reset_launch_counts()
            got = run()
            assert ops.launch_count("scan_gqa_mfma_f32") == 1 and not any(ops.launch_count(f) for f in others), what
            results += gm.compare(got, want, model, fams, what=what)
            assert (got[L == 0] == 0).all() and (got != SENTINEL).all(), f"{what}: rows of length 0 are exact zeros"
            for b in np.nonzero(L == 1)[0]:
                assert_equal(got[b], gm.expand_kv(v_rows[b, 0], H, Hkv), what=f"{what}: a row of one token returns V's row")
            for nt in (0, 1, 2):                          # both cache policies, then the rule's: the same bits every time
                assert mli.mli_tune(b"nt_loads", nt) == 0
                assert_equal(run(), got, what=f"{what}: second launch, nt_loads {nt}")
            ws, need = ops.workspace_for(B, S, D, dev, H, mfma_kv_heads=Hkv)
            assert need > 65536 and not host(ws[:65536]).any(), f"{what}: the arrival counters are zero between calls"
        if (B, S, D) == (6, 128, 256):   # |lane-group - this| <= the sum of their errors against the model: twice the bound at most
            lane_group = torch.full((B, D), SENTINEL, device=dev)
            ops.decode_scan_paged_gqa(qd, table, Ld, lane_group, H, Hkv, W, 0, ELEM["f32"], S)
            theirs = gm.compare(host(lane_group), want, model, fams, what=f"{what}: mli_decode_scan_paged_gqa")
            for (family, ours, tol), (_, lanes, _) in zip(results[-len(theirs):], theirs):
                assert ours + lanes <= 2 * tol, f"{what} | {family}: {ours:.3e} + {lanes:.3e} > 2 x {tol:.3e}"
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
        mli.mli_tune(b"nt_loads", 2)
    gm.assert_within(results, f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} part {part} {assignment}")
