"""The sliding-window paged scan with attention sinks (mli_decode_scan_paged_sinks, mli_paged_attention_lean_sinks) held to
fp32 rounding error against the sink-windowed float64 model (tests/sinks_model.py; tests/test_sinks_model_cpu.py proves that
the comparison bites).  Shapes: the smallest at which each mechanism can still go wrong --

  B, S, D         heads   pages                          (W, K)                       what it reaches
  40, 64, 64      1, 2    f32, bf16; fp8 (H 1: RPI 4)    (5,1) (16,4) (17,16)         one item per row; the hole inside a page and
                                                         (8,17) (33,20)               across a page edge; two sink pages
  24, 256, 512    1, 8    f32 (two lane loads), bf16;    (40,4) (100,20)              items that straddle the joint of the two page
                          fp8 (H 1: RPI 2)                                            runs, per-head merge; chunk_tokens 0 and 256
  20, 1024, 256   1, 2    f32, bf16                      (513,4)                      many items, many skipped pages
  24, 512, 1024   1, 8    bf16; fp8 (H 1: RPI 1)         (130,4)                      bf16 two lane loads
  8, 256, 2048    1       f32, bf16; fp8 (two lane       (100,4)                      D-split wide rows: the mask behind the
                          loads)                                                      cross-wave score reduction
  700, 128, 64    1, 2    f32                            (50,4)                       longest-first hand-out by live pages; grid
                                                                                      order too

Lengths (sinks_model.sink_lengths): 0, 1, K - 1, K, K + 1, S - 1, K + W - 1 .. K + W + 1, W + 15 .. W + 17, and the rows
whose window starts in the last sink page, in the page after it and one page further (skip 0, 0, 1).  The 8-row shape has
fewer rows than wanted lengths, so it runs twice, the lengths dealt over two vectors.

Poison: after the conversion to the page type NaN is written into the K and V slots >= L and into the gap slots [K, lo).
Every case runs once with the page-table entries of the pages wholly inside the gap pointing at a NaN-filled page and once
with them null: the two results must be bit-identical and inside the tolerance.  Tolerance: the project's rule, max(8 x the
sink-windowed oracle's own error, 16 x 2^-24) per score family (heads_model.compare), with the three head assignments of
heads_model.  For bf16 / fp8 pages the model is evaluated on the rounded pool.  K = 0 must give the bits of the windowed
entry point (on the poisoned pool: the window reads no gap slot either), and K + W >= n_sequence those of the un-windowed
one (after the gap slots have got their values back)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import f64_model as fm
import heads_model as hm
import sinks_model as sm
from accuracy_cases import base_case, dead_slot_offsets, edge_lengths, fill_pages
from gpu_util import host
from helpers import assert_equal, fp8_bits, paged_case
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

# base case outermost, so that the cached base (and its lengths) serves all its heads, page types and assignments in a row
CASES = [(seed, B, S, D, H, elem, W, K, forced, part, assignment)
         for seed, B, S, D, heads, elems, pairs, forced in sm.SINK_SHAPES for W, K in pairs
         for part in range(len(sm.sink_lengths(seed, B, S, W, K))) for H in heads for elem in elems
         if not (elem == "fp8" and H > 1) for assignment in hm.ASSIGNMENTS]


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, W, K, part):
    return base_case(seed, B, S, D, sm.sink_lengths(seed, B, S, W, K)[part])


def _tables(c, pool, elem, W, K, nan_page, dev):
    """page tables as device pointers: (all entries valid, entries of the gap's pages -> the NaN page, ... -> null)"""
    full = np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64)
    gap = sm.gap_pages(c["lengths"], full.shape[1], W, K)
    return _t(full, dev), _t(np.where(gap, nan_page.data_ptr(), full), dev), _t(np.where(gap, 0, full), dev)


def _inputs(oracle, dev, c, H, W, K, assignment, elem):
    q, kt = hm.apply_head_families(c, H, assignment)
    B, D, S = kt.shape
    L = c["lengths"]
    pool32, off = fill_pages(oracle, c, q, kt, c["v_cache"])
    gap = sm.gap_offsets(c["table"], L, S, D, W, K)
    pool, values = _poisoned_pool(pool32, np.concatenate([off, gap]), elem, dev)
    s_live = max(-(-int(L.max()) // 16) * 16, 16)
    ktm = fm.gather_pages(values, c["table"], L, s_live, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, s_live, D, 2)
    nan_page = _nan_page(D, elem, dev)
    full, to_nan, to_null = _tables(c, pool, elem, W, K, nan_page, dev)
    return SimpleNamespace(q=_t(q, dev), L=_t(L, dev), page_table=full, table_nan=to_nan, table_null=to_null, pool=pool,
                           nan_page=nan_page, B=B, S=S, D=D, H=H, W=W, K=K, lengths=L, gap=gap, gap_values=pool32[gap],
                           model=sm.model_sinks(q, ktm, v_rows, L, H, W, K),
                           oracle=sm.oracle_sinks(oracle, q, ktm, v_rows, L, H, W, K))


def _restore_gap(x, elem):
    """the gap slots get their values back (the slots >= L stay NaN): what an un-windowed scan may read"""
    if not len(x.gap):
        return
    dev = x.q.device
    values = _t(fp8_bits(x.gap_values), dev) if elem == "fp8" else _t(x.gap_values, dev).to(x.pool.dtype)
    x.pool[_t(x.gap, dev)] = values


def _scan(ops, x, elem, table=None, window=None, sinks=None):
    out = torch.full((x.B, x.D), SENTINEL, device=x.q.device)
    ops.decode_scan_paged_sinks(x.q, x.table_nan if table is None else table, x.L, out, x.H, x.W if window is None else window,
                                x.K if sinks is None else sinks, ELEM[elem], x.S)
    return host(out).copy()


def _counters_are_zero(ops, x):
    ws, need = ops.workspace_for(x.B, x.S, x.D, x.q.device, x.H)
    assert need > 65536 and not host(ws[:65536]).any(), "the arrival counters are zero between calls"


@pytest.mark.parametrize("seed,B,S,D,H,elem,W,K,forced,part,assignment", CASES)
def test_sinks_scan(oracle, mli, dev, seed, B, S, D, H, elem, W, K, forced, part, assignment):
    from min_llm_inference_amd import ops
    x = _inputs(oracle, dev, _base(seed, B, S, D, W, K, part), H, W, K, assignment, elem)
    assert x.lengths.min() == 0 and x.lengths.max() == S - 1 and 1 <= K and K + W < S
    results = []
    try:
        for ct in forced:               # 0 = the heuristic's item size at the span of sinks and window
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            what = f"B{B} S{S} D{D} H{H} W{W} K{K} {elem} chunk_tokens {ct}"
            got = _scan(ops, x, elem)
            results += hm.compare(got, x.oracle, x.model, assignment, what=what)
            assert_equal(_scan(ops, x, elem, table=x.table_null), got,
                         what=f"{what}: null page-table entries inside the gap against entries of a NaN page")
            assert_equal(_scan(ops, x, elem), got, what=f"{what}: second launch (deterministic merge, counters back at zero)")
            _counters_are_zero(ops, x)
            for nt in (0, 1):                            # both cache policies of the K / V loads
                assert mli.mli_tune(b"nt_loads", nt) == 0
                results += hm.compare(_scan(ops, x, elem), x.oracle, x.model, assignment, what=f"{what} nt_loads {nt}")
            mli.mli_tune(b"nt_loads", 2)
            if B > 512:                                  # one item per row, longest first by default: grid order too
                assert mli.mli_tune(b"scan_row_order", 0) == 0
                results += hm.compare(_scan(ops, x, elem), x.oracle, x.model, assignment, what=f"{what} grid order")
                mli.mli_tune(b"scan_row_order", 1)
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
        mli.mli_tune(b"nt_loads", 2)
        mli.mli_tune(b"scan_row_order", 1)
    hm.assert_within(results, f"B{B} S{S} D{D} H{H} W{W} K{K} {elem}")
    # K = 0 is the windowed entry point, same bits (it reads no gap slot: the pool stays poisoned, the table whole)
    want = torch.full((B, D), SENTINEL, device=dev)
    ops.decode_scan_paged_window(x.q, x.page_table, x.L, want, H, W, ELEM[elem], S)
    want = host(want).copy()
    assert np.isfinite(want).all() and (want != SENTINEL).all()
    assert_equal(_scan(ops, x, elem, table=x.page_table, sinks=0), want, what="n_sink 0 is the windowed scan")
    assert not np.array_equal(want, got), "sinks that change nothing"
    # K + W >= n_sequence is no window: the un-windowed entry point, same bits.  The gap slots hold their values again here,
    # so every row is compared as the numbers an un-windowed scan gives and not as the NaN it would have read.
    _restore_gap(x, elem)
    want = torch.full((B, D), SENTINEL, device=dev)
    if H == 1:
        ops.decode_scan_paged(x.q, x.page_table, x.L, None, want, ELEM[elem], phases=7, n_sequence=S)
    else:
        ops.decode_scan_paged_heads(x.q, x.page_table, x.L, want, H, ELEM[elem], S)
    want = host(want).copy()
    assert np.isfinite(want).all() and (want != SENTINEL).all()
    for w, k in ((W, S - W), (W, S), (S, K), (S + 1000, 1)):
        assert_equal(_scan(ops, x, elem, table=x.page_table, window=w, sinks=k), want, what=f"window {w}, n_sink {k}: no gap")


def test_a_plain_call_of_another_shape_shares_the_buffer(oracle, mli, dev):
    """One workspace serves both kinds of call: a plain scan, a scan with sinks of a different shape in the same buffer, the
    plain scan again -- same bits as before, and the result with sinks still within tolerance."""
    from min_llm_inference_amd import ops
    y = _inputs(oracle, dev, _base(503, 20, 1024, 256, 513, 4, 0), 1, 513, 4, "mixed", "f32")
    x = _inputs(oracle, dev, _base(502, 24, 256, 512, 100, 20, 0), 1, 100, 20, "flat", "f32")
    big, _ = ops.workspace_for(y.B, y.S, y.D, dev)               # grown once, for the larger need

    def plain():
        out = torch.full((x.B, x.D), SENTINEL, device=dev)
        ops.decode_scan_paged(x.q, x.page_table, x.L, None, out, 0, phases=7, n_sequence=x.S)
        assert ops.workspace_for(x.B, x.S, x.D, dev)[0].data_ptr() == big.data_ptr(), "the calls share one buffer"
        return host(out).copy().view(np.uint32)   # bit patterns: without a window the rows read the NaN put into the gap

    before = plain()
    got = _scan(ops, y, "f32")
    assert ops.workspace_for(y.B, y.S, y.D, dev)[0].data_ptr() == big.data_ptr()
    assert_equal(plain(), before, what="plain scan after a scan with sinks in the same workspace")
    hm.assert_within(hm.compare(got, y.oracle, y.model, "mixed", what="scan with sinks between two plain scans"))
    hm.assert_within(hm.compare(_scan(ops, y, "f32"), y.oracle, y.model, "mixed", what="scan with sinks after a plain scan"))
    hm.assert_within(hm.compare(_scan(ops, x, "f32"), x.oracle, x.model, "flat", what="scan with sinks of the plain scan's shape"))
    assert_equal(plain(), before, what="plain scan after a scan with sinks of its own shape")


@pytest.mark.parametrize("elem,H", [("f32", 1), ("f32", 4), ("bf16", 1), ("bf16", 4)])
def test_lean_sinks_composition(oracle, mli, dev, elem, H):
    """mli_paged_attention_lean_sinks with new rows: pages and q_output bit-identical to mli_paged_attention_lean on the same
    inputs (fill and projection are the existing launches), attention_result against the sink-windowed model of what the
    call left in memory (q_output and the pages, the appended K / V rows included), and neither what the un-windowed call
    nor what the windowed call gives."""
    from min_llm_inference_amd import ops
    seed, B, S, D, W, K = 521, 20, 256, 256, 40, 4
    L = edge_lengths(seed, B, S, (64, W + K))
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    new = [int(np.nonzero(L == n)[0][0]) for n in (2, 17, 45, 65)]
    c["n_new"] = len(new)
    c["new_batch_idx"][:len(new)] = new
    pool32 = c["pool"].copy()
    oracle.clone_to_pages(pool32, c["table"], c["inp_embedding"], c["kt_cache"], c["v_cache"], L)
    off, _, _ = dead_slot_offsets(c["table"], L, S, D)
    # (the fill rewrites whole new rows and the projection appends slot L - 1: only the slots >= L can be poisoned here)
    wdt = torch.float32 if elem == "f32" else torch.bfloat16

    def run(window, sinks):
        pool, _ = _poisoned_pool(pool32, off, elem, dev)
        d = SimpleNamespace(pool=pool, q=_t(c["q_output"], dev), out=torch.full((B, D), SENTINEL, device=dev))
        table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
        w = [_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv")]
        ops.paged_attention_lean(table, _t(L, dev), w[0], w[1], w[2], _t(c["new_batch_idx"], dev), d.q, d.out, c["n_new"], S,
                                 elem=ELEM[elem], n_heads=H, window=window, sinks=sinks)
        torch.cuda.synchronize()
        return d

    plain, cut, kept, none, whole = run(None, None), run(W, None), run(W, K), run(W, 0), run(W, S - W)
    bits = torch.int32 if elem == "f32" else torch.int16
    assert torch.equal(plain.pool.view(bits), kept.pool.view(bits)), "pages do not depend on window or sinks"
    assert_equal(host(kept.q), host(plain.q), what="q_output does not depend on window or sinks")
    assert_equal(host(whole.out), host(plain.out), what="n_sink + window = n_sequence is the un-windowed call")
    assert_equal(host(none.out), host(cut.out), what="n_sink = 0 is the windowed call")
    values = torch.nan_to_num(kept.pool.float()).cpu().numpy()
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q = host(kept.q)
    model = sm.model_sinks(q, ktm, v_rows, L, H, W, K)
    res = hm.compare(host(kept.out), sm.oracle_sinks(oracle, q, ktm, v_rows, L, H, W, K), model, "flat",
                     what=f"lean sinks composition {elem} H{H}")
    hm.assert_within(res, f"mli_paged_attention_lean_sinks {elem} H{H}")
    assert not np.array_equal(host(kept.out), host(plain.out)), "a window of 40 with 4 sinks gives what no window gives"
    assert not np.array_equal(host(kept.out), host(cut.out)), "4 sinks give what the window alone gives"


@pytest.mark.parametrize("elem,D", [("f32", 1024), ("bf16", 4096)])
def test_rows_split_across_the_waves_at_the_other_lane_counts(oracle, mli, dev, elem, D):
    """One head on rows of more than two lane loads (the four waves split the row, DS): SINK_SHAPES has emb_dim 2048, which is two
    lane loads per wave on fp32 pages and one on bf16 pages.  Here the other two, with sinks (K 4) and without (K 0: the windowed
    kernel), under both nt_loads settings (tests/kernel_coverage.json):
      f32 D 1024:  window_decode_scan_kernel<ElemF32, 1, NT, 8, true, 1, SINK>
      bf16 D 4096: window_decode_scan_kernel<ElemBF16, 2, NT, 4, true, 1, SINK>"""
    from min_llm_inference_amd import ops
    seed, B, S, W = 507, 8, 128, 40
    results = []
    try:
        for K in (4, 0):
            for part in range(len(sm.sink_lengths(seed, B, S, W, 4))):
                x = _inputs(oracle, dev, _base(seed, B, S, D, W, 4, part), 1, W, K, "flat", elem)
                got = {}
                for nt in (0, 1):
                    assert mli.mli_tune(b"nt_loads", nt) == 0
                    what = f"B{B} S{S} D{D} H1 W{W} K{K} {elem} part {part} nt_loads {nt}"
                    got[nt] = _scan(ops, x, elem)
                    assert (got[nt][x.lengths == 0] == 0).all(), f"{what}: rows of length 0"
                    results += hm.compare(got[nt], x.oracle, x.model, "flat", what=what)
                assert_equal(got[1], got[0], what=f"{what}: nt_loads 1 against nt_loads 0")
                assert_equal(_scan(ops, x, elem), got[1], what=f"{what}: second launch")
    finally:
        mli.mli_tune(b"nt_loads", 2)
    hm.assert_within(results, f"B{B} S{S} D{D} H1 W{W} {elem}")
