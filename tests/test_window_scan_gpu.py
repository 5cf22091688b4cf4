"""The sliding-window paged scan (mli_decode_scan_paged_window, mli_paged_attention_lean_window) held to fp32 rounding
error against the windowed float64 model (tests/window_model.py; tests/test_window_model_cpu.py proves that the comparison
bites).  Shapes: the smallest at which each mechanism can still go wrong --

  B, S, D         heads   pages                          windows           what it reaches
  40, 64, 64      1, 2    f32, bf16; fp8 (H 1: RPI 4)    1, 5, 16, 17, 33  one item per row; both masks in one page; window on
                                                                           and across a page edge; W = 1 exact
  24, 256, 512    1, 8    f32 (two lane loads), bf16;    40, 100, 255      several items from a shifted origin, per-head merge;
                          fp8 (H 1: RPI 2)                                 chunk_tokens 0 and 256
  20, 1024, 256   1, 2    f32, bf16                      100, 513          first item not the row's first page; many items
  24, 512, 1024   1, 8    bf16; fp8 (H 1: RPI 1)         130               bf16 two lane loads; chunk_tokens 0, 256
  8, 256, 2048    1       f32, bf16; fp8 (two lane       100               D-split wide rows: the low mask in the cross-wave
                          loads)                                           score reduction
  700, 128, 64    1, 2    f32                            50                longest-first hand-out with windowed lengths; grid
                                                                           order too
  16, 4096, 512   1, 4    bf16                           1024              chunk_tokens 64 and 1024

Lengths (window_model.window_lengths): accuracy_cases.edge_lengths with W among its chunk edges, plus W + 15, W + 16, W + 17
(with W + 1: windows that start 15, 0 and 1 slots into a page); 0 and S - 1 are asserted.  The 8-row shape has fewer rows
than wanted lengths, so it runs twice, the lengths dealt over two vectors.

Poison: after the conversion to the page type NaN is written into the K and V slots >= L and the slots < lo of the first
live page.  Every case runs once with the page-table entries below the first live page pointing at a NaN-filled page and
once with them null: the two results must be bit-identical and inside the tolerance.  (The comparison of W >= n_sequence
with the un-windowed entry point comes last, after the slots below the window have got their values back.)  Tolerance:
the project's rule, max(8 x the windowed oracle's own error, 16 x 2^-24) per score family (heads_model.compare), with the
three head assignments of heads_model.  For bf16 / fp8 pages the model is evaluated on the rounded pool."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import f64_model as fm
import heads_model as hm
import window_model as wm
from accuracy_cases import base_case, dead_slot_offsets, edge_lengths, fill_pages
from gpu_util import host
from helpers import assert_equal, fp8_bits, fp8_decode, paged_case

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
ELEM = {"f32": 0, "bf16": 1, "fp8": 2}
ESIZE = {"f32": 4, "bf16": 2, "fp8": 1}
# base case outermost, so that the cached base (and its lengths) serves all its heads, page types and assignments in a row
CASES = [(seed, B, S, D, H, elem, W, forced, chunks, part, assignment)
         for seed, B, S, D, heads, elems, windows, forced, chunks in wm.WINDOW_SHAPES for W in windows
         for part in range(len(wm.window_lengths(seed, B, S, W, chunks))) for H in heads for elem in elems
         if not (elem == "fp8" and H > 1) for assignment in hm.ASSIGNMENTS]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, W, chunks, part):
    return base_case(seed, B, S, D, wm.window_lengths(seed, B, S, W, chunks)[part])


@functools.lru_cache(maxsize=1)
def _base_with(seed, B, S, D, lengths):
    return base_case(seed, B, S, D, np.asarray(lengths, np.int32))


def _poisoned_pool(pool32, off, elem, dev):
    """(device pool of the page type with NaN at the element offsets `off`, the float32 values the other slots hold)"""
    offs = _t(off, dev) if len(off) else None
    if elem == "fp8":
        bits = fp8_bits(pool32)
        pool, values = _t(bits, dev), fp8_decode(bits)
        if offs is not None:
            pool[offs] = 0x7F
        return pool, values
    t = _t(pool32, dev)
    if elem == "f32":
        pool, values = t, pool32
        if offs is not None:
            pool[offs] = float("nan")
    else:
        pool = t.to(torch.bfloat16)
        values = pool.float().cpu().numpy()
        if offs is not None:
            pool.view(torch.int16)[offs] = 0x7FC0
    return pool, values


def _nan_page(D, elem, dev):
    if elem == "fp8":
        return torch.full((16 * 3 * D,), 0x7F, dtype=torch.uint8, device=dev)
    return torch.full((16 * 3 * D,), float("nan"), dtype=torch.float32 if elem == "f32" else torch.bfloat16, device=dev)


def _tables(c, pool, elem, W, nan_page, dev):
    """page tables as device pointers: (all entries valid, entries below the first live page -> the NaN page, ... -> null)"""
    full = np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64)
    p0 = wm.window_lo(c["lengths"], W) // 16
    below = np.arange(full.shape[1])[None, :] < p0[:, None]
    return _t(full, dev), _t(np.where(below, nan_page.data_ptr(), full), dev), _t(np.where(below, 0, full), dev)


def _inputs(oracle, dev, c, H, W, assignment, elem):
    q, kt = hm.apply_head_families(c, H, assignment)
    B, D, S = kt.shape
    L = c["lengths"]
    pool32, off = fill_pages(oracle, c, q, kt, c["v_cache"])
    low = wm.low_dead_offsets(c["table"], L, S, D, W)
    pool, values = _poisoned_pool(pool32, np.concatenate([off, low]), elem, dev)
    s_live = max(-(-int(L.max()) // 16) * 16, 16)
    ktm = fm.gather_pages(values, c["table"], L, s_live, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, s_live, D, 2)
    nan_page = _nan_page(D, elem, dev)
    full, to_nan, to_null = _tables(c, pool, elem, W, nan_page, dev)
    return SimpleNamespace(q=_t(q, dev), L=_t(L, dev), page_table=full, table_nan=to_nan, table_null=to_null, pool=pool,
                           nan_page=nan_page, B=B, S=S, D=D, H=H, W=W, lengths=L, v_rows=v_rows, low=low,
                           low_values=pool32[low],
                           model=wm.model_window(q, ktm, v_rows, L, H, W),
                           oracle=wm.oracle_window(oracle, q, ktm, v_rows, L, H, W))


def _restore_below_window(x, elem):
    """the slots below the window get their values back (the slots >= L stay NaN): what an un-windowed scan may read"""
    if not len(x.low):
        return
    dev = x.q.device
    if elem == "fp8":
        values = _t(fp8_bits(x.low_values), dev)
    else:
        values = _t(x.low_values, dev).to(x.pool.dtype)
    x.pool[_t(x.low, dev)] = values


def _scan(ops, x, elem, table=None, window=None, n_heads=None):
    out = torch.full((x.B, x.D), SENTINEL, device=x.q.device)
    ops.decode_scan_paged_window(x.q, x.table_nan if table is None else table, x.L, out, x.H if n_heads is None else n_heads,
                                 x.W if window is None else window, ELEM[elem], x.S)
    return host(out).copy()


def _counters_are_zero(ops, x):
    ws, need = ops.workspace_for(x.B, x.S, x.D, x.q.device, x.H)
    assert need > 65536 and not host(ws[:65536]).any(), "the arrival counters are zero between calls"


@pytest.mark.parametrize("seed,B,S,D,H,elem,W,forced,chunks,part,assignment", CASES)
def test_window_scan(oracle, mli, dev, seed, B, S, D, H, elem, W, forced, chunks, part, assignment):
    from min_llm_inference_amd import ops
    x = _inputs(oracle, dev, _base(seed, B, S, D, W, chunks, part), H, W, assignment, elem)
    assert x.lengths.min() == 0 and x.lengths.max() == S - 1
    results = []
    try:
        for ct in forced:               # 0 = the heuristic's item size at the window's span
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            what = f"B{B} S{S} D{D} H{H} W{W} {elem} chunk_tokens {ct}"
            got = _scan(ops, x, elem)
            results += hm.compare(got, x.oracle, x.model, assignment, what=what)
            assert_equal(_scan(ops, x, elem, table=x.table_null), got,
                         what=f"{what}: null page-table entries below the window against entries of a NaN page")
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
            if W == 1:                                   # p = exp(0) = 1, l = 1: V's row L - 1, bit for bit
                live = x.lengths > 0
                want = x.v_rows[np.nonzero(live)[0], x.lengths[live] - 1].astype(np.float32)
                assert_equal(got[live], want, what=f"{what}: W = 1 is the newest V row")
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
        mli.mli_tune(b"nt_loads", 2)
        mli.mli_tune(b"scan_row_order", 1)
    hm.assert_within(results, f"B{B} S{S} D{D} H{H} W{W} {elem}")
    # W >= n_sequence is no window: the existing entry point, same bits.  The slots below the window hold their values
    # again here, so every row is compared as the numbers an un-windowed scan gives and not as the NaN it would have read.
    _restore_below_window(x, elem)
    want = torch.full((B, D), SENTINEL, device=dev)
    if H == 1:
        ops.decode_scan_paged(x.q, x.page_table, x.L, None, want, ELEM[elem], phases=7, n_sequence=S)
    else:
        ops.decode_scan_paged_heads(x.q, x.page_table, x.L, want, H, ELEM[elem], S)
    want = host(want).copy()
    assert np.isfinite(want).all() and (want != SENTINEL).all()
    for no_window in (S, S + 1000):
        assert_equal(_scan(ops, x, elem, table=x.page_table, window=no_window), want, what=f"window {no_window} >= n_sequence")


@pytest.mark.parametrize("assignment", hm.ASSIGNMENTS)
@pytest.mark.parametrize("H,elem,W", [(1, "f32", 100), (2, "bf16", 513)])
def test_window_scan_with_rows_of_S_tokens(oracle, mli, dev, H, elem, W, assignment):
    """The S = 1024 shape with its two long random rows made full: L == n_sequence, all S / 16 pages present, the window
    [S - W, S) (the scan clamps with min(L, S); every other case stops at S - 1)."""
    from min_llm_inference_amd import ops
    seed, B, S, D, _, _, _, _, chunks = wm.WINDOW_SHAPES[2]
    L = wm.window_lengths(seed, B, S, W, chunks)[0].copy()
    rows = np.nonzero((L >= 3 * S // 4) & (L < S - 2))[0][:2]
    assert len(rows) == 2
    L[rows] = S
    x = _inputs(oracle, dev, _base_with(seed, B, S, D, tuple(L.tolist())), H, W, assignment, elem)
    assert x.lengths.min() == 0 and x.lengths.max() == S and (x.lengths == S).sum() == 2
    what = f"B{B} S{S} D{D} H{H} W{W} {elem}, rows of S tokens"
    got = _scan(ops, x, elem)
    results = hm.compare(got, x.oracle, x.model, assignment, what=what)
    assert_equal(_scan(ops, x, elem, table=x.table_null), got, what=f"{what}: null page-table entries below the window")
    assert_equal(_scan(ops, x, elem), got, what=f"{what}: second launch")
    _counters_are_zero(ops, x)
    hm.assert_within(results, what)


def test_a_plain_call_of_another_shape_shares_the_buffer(oracle, mli, dev):
    """One workspace serves both kinds of call: a plain scan, a windowed scan of a different shape in the same buffer, the
    plain scan again -- same bits as before, and the windowed result still within tolerance."""
    from min_llm_inference_amd import ops
    y = _inputs(oracle, dev, _base(403, 20, 1024, 256, 513, (64,), 0), 1, 513, "mixed", "f32")
    x = _inputs(oracle, dev, _base(402, 24, 256, 512, 100, (64,), 0), 1, 100, "flat", "f32")
    big, _ = ops.workspace_for(y.B, y.S, y.D, dev)               # grown once, for the larger need

    def plain():
        out = torch.full((x.B, x.D), SENTINEL, device=dev)
        ops.decode_scan_paged(x.q, x.page_table, x.L, None, out, 0, phases=7, n_sequence=x.S)
        assert ops.workspace_for(x.B, x.S, x.D, dev)[0].data_ptr() == big.data_ptr(), "the calls share one buffer"
        return host(out).copy().view(np.uint32)   # bit patterns: without a window the rows read the NaN put below it

    before = plain()
    got = _scan(ops, y, "f32")
    assert ops.workspace_for(y.B, y.S, y.D, dev)[0].data_ptr() == big.data_ptr()
    assert_equal(plain(), before, what="plain scan after a windowed scan in the same workspace")
    hm.assert_within(hm.compare(got, y.oracle, y.model, "mixed", what="windowed scan between two plain scans"))
    hm.assert_within(hm.compare(_scan(ops, y, "f32"), y.oracle, y.model, "mixed", what="windowed scan after a plain scan"))
    hm.assert_within(hm.compare(_scan(ops, x, "f32"), x.oracle, x.model, "flat", what="windowed scan of the plain scan's shape"))
    assert_equal(plain(), before, what="plain scan after a windowed scan of its own shape")


@pytest.mark.parametrize("elem,H", [("f32", 1), ("f32", 4), ("bf16", 1), ("bf16", 4)])
def test_lean_window_composition(oracle, mli, dev, elem, H):
    """mli_paged_attention_lean_window with new rows: pages and q_output bit-identical to the un-windowed call on the same
    inputs (fill and projection are the existing launches), attention_result against the windowed model of what the call
    left in memory (q_output and the pages, the appended K / V rows included), and not what the un-windowed call gives."""
    from min_llm_inference_amd import ops
    seed, B, S, D, W = 421, 20, 256, 256, 40
    L = edge_lengths(seed, B, S, (64, W))
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    new = [b for b in range(B) if int(L[b]) in (2, 17, 41, 65)]
    assert len(new) == 4
    c["n_new"] = len(new)
    c["new_batch_idx"][:len(new)] = new
    pool32 = c["pool"].copy()
    oracle.clone_to_pages(pool32, c["table"], c["inp_embedding"], c["kt_cache"], c["v_cache"], L)
    off, _, _ = dead_slot_offsets(c["table"], L, S, D)
    # (the fill rewrites whole new rows and the projection appends slot L - 1: only the slots >= L can be poisoned here)
    wdt = torch.float32 if elem == "f32" else torch.bfloat16

    def run(window):
        pool, _ = _poisoned_pool(pool32, off, elem, dev)
        d = SimpleNamespace(pool=pool, q=_t(c["q_output"], dev), out=torch.full((B, D), SENTINEL, device=dev))
        table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
        w = [_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv")]
        ops.paged_attention_lean(table, _t(L, dev), w[0], w[1], w[2], _t(c["new_batch_idx"], dev), d.q, d.out, c["n_new"], S,
                                 elem=ELEM[elem], n_heads=H, window=window)
        torch.cuda.synchronize()
        return d

    plain, cut, whole = run(None), run(W), run(S)
    bits = torch.int32 if elem == "f32" else torch.int16
    assert torch.equal(plain.pool.view(bits), cut.pool.view(bits)), "pages do not depend on the window"
    assert_equal(host(cut.q), host(plain.q), what="q_output does not depend on the window")
    assert_equal(host(whole.out), host(plain.out), what="window = n_sequence is the un-windowed call")
    values = torch.nan_to_num(cut.pool.float()).cpu().numpy()
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q = host(cut.q)
    model = wm.model_window(q, ktm, v_rows, L, H, W)
    res = hm.compare(host(cut.out), wm.oracle_window(oracle, q, ktm, v_rows, L, H, W), model, "flat",
                     what=f"lean window composition {elem} H{H}")
    hm.assert_within(res, f"mli_paged_attention_lean_window {elem} H{H}")
    assert not np.array_equal(host(cut.out), host(plain.out)), "a window of 40 gives what no window gives"
