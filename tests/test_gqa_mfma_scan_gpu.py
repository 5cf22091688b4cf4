"""The grouped-query scan on matrix instructions (mli_decode_scan_paged_gqa_mfma) held to fp32 rounding error against
the float64 model on the expanded operands (tests/gqa_model.py), evaluated on the rounded bf16 pool.

  B, S, D         H / Hkv (g), hd    windows    what it reaches
  6, 128, 256     4/2 (2), 64        0, 40      a shape the lane-group scan also takes (mli_decode_scan_paged_gqa is run beside it)
  5, 256, 2048    16/4 (4), 128      0, 100     a wide row
  5, 256, 2048    16/2 (8), 128      0          the largest group
  5, 256, 2048    16/16 (1), 128     0          g = 1 at a width the multi-head scan refuses
  5, 128, 448     7/1 (7), 64        0, 17      odd g, padded tile columns, hd 64
  4, 1024, 1024   8/2 (4), 128       0, 513     many items per row

Lengths: accuracy_cases.edge_lengths up to S with 64 and W among the forced edges, dealt over as many vectors of B rows as it
takes; 0, 1, 16, 17, S - 1 and S are asserted.  Items of 64 tokens forced (several per row, the last arriver's merge) and the
heuristic's; both cache policies of the K / V loads.  NaN is written into the K / V slots >= L, the slots below the window, the
x segment and the K / V columns >= Hkv * hd of every owned slot, and the page-table entries of the pages wholly below the window
point at a NaN page.  Tolerance: f64_model.tolerance per score family, unchanged.  That bound is what holds the bf16 splitting to
account: the same inputs through a float64 model whose q and probabilities keep ONE bf16 part must exceed it (asserted here, in
numpy), so a kernel that rounds either operand fails."""
import functools

import numpy as np
import pytest
import torch

import f64_model as fm
import gqa_model as gm
import heads_model as hm
import sinks_model as sm
from accuracy_cases import base_case, edge_lengths, fill_pages
from gpu_util import host
from helpers import assert_equal
from test_gqa_scan_gpu import _device_tables, _unread_offsets
from test_window_scan_gpu import ELEM, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

SHAPES = [(701, 6, 128, 256, 4, 2, (0, 40)), (702, 5, 256, 2048, 16, 4, (0, 100)), (703, 5, 256, 2048, 16, 2, (0,)),
          (704, 5, 256, 2048, 16, 16, (0,)), (705, 5, 128, 448, 7, 1, (0, 17)), (706, 4, 1024, 1024, 8, 2, (0, 513))]


def _length_vectors(seed, B, S, W):
    rows = B * -(-18 // B)      # edge_lengths forces at most 14 edges and two long rows
    return edge_lengths(seed, rows, S, (64, W) if W else (64,), top=S).reshape(-1, B)


CASES = [(seed, B, S, D, H, Hkv, W, part, assignment) for seed, B, S, D, H, Hkv, windows in SHAPES for W in windows
         for part in range(len(_length_vectors(seed, B, S, W))) for assignment in ("mixed", "offsets")]


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, W, part):
    return base_case(seed, B, S, D, _length_vectors(seed, B, S, W)[part])


def _bf16_one_part(a):
    return (np.asarray(a, np.float32).view(np.uint32) & 0xFFFF0000).view(np.float32)


def _one_part_model(q, kt, v, L, H, Hkv):
    """float64 attention (no window) in which q and the probabilities keep one bf16 part"""
    kx, vx, D = gm.expand_kv(kt, H, Hkv, 1), gm.expand_kv(v, H, Hkv, 2), q.shape[1]
    o = np.zeros(q.shape, np.float64)
    for h in range(H):
        sl = hm.head_slice(h, H, D)
        p = fm.softmax(fm.scores(_bf16_one_part(q[:, sl]), kx[:, sl, :], L), L)
        o[:, sl] = fm.attend(_bf16_one_part(p), vx[:, :, sl], L)
    return o


@pytest.mark.parametrize("seed,B,S,D,H,Hkv,W,part,assignment", CASES)
def test_gqa_mfma_scan(oracle, mli, dev, seed, B, S, D, H, Hkv, W, part, assignment):
    from min_llm_inference_amd import ops
    every = _length_vectors(seed, B, S, W)
    assert {0, 1, 16, 17, 63, 64, 65, S - 1, S} | ({W} if W else set()) <= set(every.reshape(-1).tolist())
    c = _base(seed, B, S, D, W, part)
    L, hd = c["lengths"], D // H
    q, kt = gm.apply_gqa_families(c, H, Hkv, assignment)
    pool32, off = fill_pages(oracle, c, q, kt, c["v_cache"])
    pages = c["table"][c["table"] >= 0].astype(np.int64)
    x_seg = (pages[:, None, None] + (np.arange(16) * 3 * D)[None, :, None] + np.arange(D)[None, None, :]).reshape(-1)
    gap = sm.gap_offsets(c["table"], L, S, D, W, 0) if W else np.zeros(0, np.int64)
    pool, values = _poisoned_pool(pool32, np.concatenate([off, gap, x_seg, _unread_offsets(c, D, Hkv * hd)]), "bf16", dev)
    s_live = max(-(-int(L.max()) // 16) * 16, 16)
    ktm = fm.gather_pages(values, c["table"], L, s_live, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, s_live, D, 2)
    model, want = gm.model_gqa(q, ktm, v_rows, L, H, Hkv, W), gm.oracle_gqa(oracle, q, ktm, v_rows, L, H, Hkv, W)
    fams = gm.head_families(assignment, H, Hkv)
    nan_page = _nan_page(D, "bf16", dev)
    _, table, _ = _device_tables(c, pool, "bf16", W, 0, nan_page, dev)
    qd, Ld = _t(q, dev), _t(L, dev)

    def run():
        out = torch.full((B, D), SENTINEL, device=dev)
        ops.decode_scan_paged_gqa_mfma(qd, table, Ld, out, H, Hkv, W, S)
        return host(out).copy()

    others = [f for f in ops.launch_families() if f.startswith("scan_") and f != "scan_gqa_mfma"]
    assert len(others) >= 11, others
    results = []
    try:
        for ct in (64, 0):
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            what = f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} part {part} {assignment} chunk_tokens {ct}"
            ops.reset_launch_counts()
            got = run()
            assert ops.launch_count("scan_gqa_mfma") == 1 and not any(ops.launch_count(f) for f in others), what
            results += gm.compare(got, want, model, fams, what=what)
            assert (got[L == 0] == 0).all() and (got != SENTINEL).all(), f"{what}: rows of length 0 are exact zeros"
            for b in np.nonzero(L == 1)[0]:
                assert_equal(got[b], gm.expand_kv(v_rows[b, 0], H, Hkv), what=f"{what}: a row of one token returns V's row")
            for nt in (0, 1, 2):                          # both cache policies, then the rule's: the same bits every time
                assert mli.mli_tune(b"nt_loads", nt) == 0
                assert_equal(run(), got, what=f"{what}: second launch, nt_loads {nt}")
            ws, need = ops.workspace_for(B, S, D, dev, H, mfma_kv_heads=Hkv)
            assert need > 65536 and not host(ws[:65536]).any(), f"{what}: the arrival counters are zero between calls"
        if (B, S, D) == (6, 128, 256):
            lane_group = torch.full((B, D), SENTINEL, device=dev)
            ops.decode_scan_paged_gqa(qd, table, Ld, lane_group, H, Hkv, W, 0, ELEM["bf16"], S)
            results += gm.compare(host(lane_group), want, model, fams, what=f"{what}: mli_decode_scan_paged_gqa")
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
        mli.mli_tune(b"nt_loads", 2)
    gm.assert_within(results, f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} part {part} {assignment}")
    if W == 0:
        rounded = gm.compare(_one_part_model(q, ktm, v_rows, L, H, Hkv), want, model, fams, what="one bf16 part", report=lambda s: None)
        assert any(worst > tol for _, worst, tol in rounded), "one bf16 part of q and of the probabilities stays inside the tolerance"
