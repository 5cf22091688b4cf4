"""The causal multi-query paged scan (mli_prompt_scan_paged) held to fp32 rounding error against the float64 model
on the virtual rows (tests/prompt_model.py; tests/test_prompt_model_cpu.py proves that the comparison bites), and cross-checked
against the decode scans run on the same virtual rows.

Shapes (prompt_model.SHAPES, n_sequence 128): the smallest that reach every kernel variant -- fp32 D 64 (a partly filled lane
load), 256, 512 (two lane loads); bf16 D 128, 1024; 4 heads at head_dim 32 and 64; 8 heads on 2 and on 1 K/V heads -- each
plain, under window 40, window 40 + 4 sinks and window 16 (a single page).  Segments (prompt_model.segments_for, by the
variant's mli_prompt_scan_tq): counts 1, TQ - 1, TQ, TQ + 1, 2 TQ + 1; first positions 0, 15, 16, 17; a query at n_sequence - 1;
two segments of one row; rows in permuted order.  Score families: accuracy_cases' six with one head, heads_model's three
assignments with several.

  tolerance   f64_model.tolerance (8 x) of the fp32 CPU oracle's own error on the same virtual rows, per score family
  poison      every K / V slot above a row's last scored position is NaN, every page beyond it a NaN page; results stay finite
  out         rows of `out` that belong to no query (a hole between two segments, a tail) keep their poison
  cross-check every query within twice the bound of mli_decode_scan_paged_gqa (which is the plain, heads, window and sinks
              scan where the form has no more) on the virtual row of length t + 1
  counter     one "scan_prompt" launch, no decode scan"""
import functools

import numpy as np
import pytest
import torch

import f64_model as fm
import gqa_model as gm
import heads_model as hm
import prompt_model as pm
from accuracy_cases import apply_family, base_case, fill_pages
from gpu_util import host
from helpers import assert_equal
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

HOLE_AFTER, HOLE, TAIL = 3, 2, 1     # `out` rows of no query: HOLE rows after segment HOLE_AFTER, TAIL rows at the end


@functools.lru_cache(maxsize=2)
def _case(seed, D, tq):
    segs, lengths = pm.segments_for(tq)
    return segs, lengths, base_case(seed, len(lengths), pm.S, D, lengths)


def _assignments(H):
    return pm.FAMILIES if H == 1 else hm.ASSIGNMENTS


def _operands(c, H, Hkv, assignment):
    if H == 1:
        q, kt = apply_family(c, assignment)
        return q, kt, (assignment,)
    q, kt = gm.apply_gqa_families(c, H, Hkv, assignment)
    return q, kt, gm.head_families(assignment, H, Hkv)


def _distance(a, b, model):
    """[n, H]: max_d |a - b| over the head's columns in units of the model's condition scale"""
    out = np.zeros((a.shape[0], model.H))
    for h in range(model.H):
        sl = hm.head_slice(h, model.H, model.D)
        out[:, h] = np.abs(a[:, sl].astype(np.float64) - b[:, sl]).max(axis=1) / model.o_scale[:, h]
    return out


@pytest.mark.parametrize("W,K", pm.FORMS)
@pytest.mark.parametrize("seed,D,H,Hkv,elem", pm.SHAPES)
def test_prompt_scan(oracle, mli, dev, seed, D, H, Hkv, elem, W, K):
    from min_llm_inference_amd import ops
    S = pm.S
    tq = ops.prompt_scan_tq(D, H, ELEM[elem])
    segs, lengths, c = _case(seed, D, tq)
    rows, pos = pm.queries(segs)
    n = len(rows)
    counts = [cnt for _, _, cnt in segs]
    dense = np.concatenate([[0], np.cumsum(counts)[:-1]])
    offsets = dense + np.where(np.arange(len(segs)) > HOLE_AFTER, HOLE, 0)
    where = np.concatenate([np.arange(o, o + cnt) for o, cnt in zip(offsets, counts)])     # the out row of every query
    n_rows = n + HOLE + TAIL
    nobody = np.setdiff1d(np.arange(n_rows), where)
    assert len(nobody) == HOLE + TAIL
    seg_arrays = tuple(_t(np.asarray(a, np.int32), dev) for a in ([r for r, _, _ in segs], [f for _, f, _ in segs], counts, offsets))
    seg_arrays += (max(counts),)
    nan_page = _nan_page(D, elem, dev)
    results = []
    for assignment in _assignments(H):
        what = f"D{D} H{H}/{Hkv} {elem} W{W} K{K} TQ{tq} {assignment}"
        q, kt, fams = _operands(c, H, Hkv, assignment)
        pool32, off = fill_pages(oracle, c, q, kt, c["v_cache"])
        pool, values = _poisoned_pool(pool32, off, elem, dev)                 # NaN above every row's last scored position
        ktm = fm.gather_pages(values, c["table"], lengths, S, D, 1).transpose(0, 2, 1)
        v_rows = fm.gather_pages(values, c["table"], lengths, S, D, 2)
        table = np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], nan_page.data_ptr()).astype(np.int64)
        assert (c["table"] < 0).any(), "a page beyond a row's last scored position"
        qv = pm.query_vectors(q, rows, pos)
        model = pm.model_prompt(qv, ktm, v_rows, rows, pos, H, Hkv, W, K)
        o_or = pm.oracle_prompt(oracle, qv, ktm, v_rows, rows, pos, H, Hkv, W, K)

        q_dev = torch.full((n_rows, D), float("nan"), device=dev)
        q_dev[_t(where, dev)] = _t(qv, dev)
        out = torch.full((n_rows, D), SENTINEL, device=dev)
        ops.reset_launch_counts()
        ops.prompt_scan_paged(q_dev, _t(table, dev), None, out, len(lengths), S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W,
                              sinks=K, seg_arrays=seg_arrays)
        counts_now = {f: ops.launch_count(f) for f in ("scan_prompt", "scan_chunked", "scan_heads_window", "scan_equal_shares")}
        assert counts_now == {"scan_prompt": 1, "scan_chunked": 0, "scan_heads_window": 0, "scan_equal_shares": 0}, counts_now
        got_all = host(out).copy()
        assert (got_all[nobody] == SENTINEL).all(), f"{what}: an out row of no query was written"
        got = got_all[where]
        assert np.isfinite(got).all() and (got != SENTINEL).any(axis=1).all(), what
        res = gm.compare(got, o_or, model, fams, what=what)
        results += res

        # the decode scans on the virtual rows: row i = the pages of rows[i] with length pos[i] + 1
        vq, vt, vL = _t(qv, dev), _t(table[rows], dev), _t((pos + 1).astype(np.int32), dev)
        ref = torch.full((n, D), SENTINEL, device=dev)
        ops.decode_scan_paged_gqa(vq, vt, vL, ref, H, Hkv, W, K, ELEM[elem], S)
        ref = host(ref)
        assert np.isfinite(ref).all(), what
        d = _distance(got, ref, model)
        for family, _, tol in res:
            cols = [h for h in range(H) if fams[h] == family]
            worst = float(d[:, cols].max())
            print(f"PROMPT {what} | {family}: {worst:.3e} from the decode scan on the virtual rows, twice the bound {2 * tol:.3e}")
            assert worst <= 2 * tol, (what, family, worst, tol)

        out2 = torch.full((n_rows, D), SENTINEL, device=dev)
        ops.prompt_scan_paged(q_dev, _t(table, dev), None, out2, len(lengths), S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W,
                              sinks=K, seg_arrays=seg_arrays)
        assert_equal(host(out2), got_all, what=f"{what}: second launch")
    gm.assert_within(results, f"D{D} H{H}/{Hkv} {elem} W{W} K{K}")


def test_segments_outside_the_batch_or_the_sequence_are_skipped(oracle, mli, dev):
    """Device values never fault: a segment with a row outside the batch, a position outside the sequence, a negative count or
    an offset outside `out` writes nothing; the good segment beside them gives the same bits as alone."""
    from min_llm_inference_amd import ops
    seed, D, H, Hkv, elem = pm.SHAPES[1]
    S = pm.S
    tq = ops.prompt_scan_tq(D, H, ELEM[elem])
    segs, lengths, c = _case(seed, D, tq)
    q, kt = apply_family(c, "flat")
    pool32, off = fill_pages(oracle, c, q, kt, c["v_cache"])
    pool, _ = _poisoned_pool(pool32, off, elem, dev)
    nan_page = _nan_page(D, elem, dev)
    table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], nan_page.data_ptr()).astype(np.int64), dev)
    good = (3, 0, 2 * tq + 1)
    n = good[2]
    qd = _t(pm.query_vectors(q, *pm.queries([good])), dev)
    alone = torch.full((n, D), SENTINEL, device=dev)
    ops.prompt_scan_paged(qd, table, [good], alone, len(lengths), S, ELEM[elem])
    B = len(lengths)
    # (row, first, count, offset): a row outside the batch, positions outside the sequence, counts below one, offsets whose
    # segment would lie outside `out`
    bad = [(-1, 0, 2, 0), (B, 0, 2, 0), (1, -1, 2, 0), (1, S - 1, 2, 0), (1, 0, -3, 0), (1, 0, 0, 0), (1, 0, 2, n - 1), (1, 0, 2, -2)]
    arrays = [[good[0]] + [b[0] for b in bad], [good[1]] + [b[1] for b in bad], [good[2]] + [b[2] for b in bad],
              [0] + [b[3] for b in bad]]
    seg_arrays = tuple(_t(np.asarray(a, np.int32), dev) for a in arrays) + (n,)
    out = torch.full((n, D), SENTINEL, device=dev)
    ops.prompt_scan_paged(qd, table, None, out, B, S, ELEM[elem], seg_arrays=seg_arrays)
    torch.cuda.synchronize()
    assert_equal(host(out), host(alone), what="a good segment among refused ones")
    assert np.isfinite(host(out)).all()


@pytest.mark.parametrize("elem,D", [("f32", 128), ("f32", 72), ("bf16", 256)])
def test_project_q_is_the_decode_projection_at_any_position(oracle, mli, dev, elem, D):
    """mli_prompt_project_q at position L - 1 of every row gives the bits of the decode projection's q_output (fp32: every
    fp32 GEMM kernel is the same k-ordered chain; bf16: the widened form, mli_tune bf16_native_mfma 0), in permuted segment
    order and beside a hole in q; rows of q that belong to no position are left alone."""
    from helpers import paged_case
    from min_llm_inference_amd import ops
    B, S = 9, 64
    L = np.asarray([1, 2, 15, 16, 17, 33, 48, 63, 5], np.int32)
    c = paged_case(811, B, S, D, conditioned=True, lengths=L)
    pool32 = c["pool"].copy()
    oracle.clone_to_pages(pool32, c["table"], c["inp_embedding"], c["kt_cache"], c["v_cache"], L)
    pool, _ = _poisoned_pool(pool32, np.zeros(0, np.int64), elem, dev)
    table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
    wdt = torch.float32 if elem == "f32" else torch.bfloat16
    wk, wq, wv = (_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv"))
    order = [4, 0, 8, 2, 7, 1, 3, 6, 5]
    segments = [(b, int(L[b]) - 1, 1) for b in order]
    got = host(ops.prompt_project_q(table, segments, wq, B, S, ELEM[elem]))
    want = torch.full((B, D), SENTINEL, device=dev)
    try:
        assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        ops.get_latest_k_q_v_paged_lean(table, _t(L, dev), wk, wq, wv, want, S, elem=ELEM[elem])
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)
    assert_equal(got, host(want)[order], what=f"{elem} D{D}: q of position L - 1")
    # earlier positions: against float64 x . Wq on what the pages hold, at the fp32 chain's own bound D 2^-24 sum |x w|
    b = 7
    seg = [(b, 0, int(L[b]))]
    q = host(ops.prompt_project_q(table, seg, wq, B, S, ELEM[elem])).astype(np.float64)
    x = c["inp_embedding"][b, :L[b]]
    w = c["wq"]
    if elem == "bf16":
        from helpers import bf16_round
        x, w = bf16_round(x), bf16_round(w)
    exact = x.astype(np.float64) @ w.astype(np.float64)
    bound = D * 2.0 ** -24 * (np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64))
    assert (np.abs(q - exact) <= bound).all(), float((np.abs(q - exact) / bound).max())
