"""The multi-head paged scan with grouped-query attention (mli_decode_scan_paged_gqa, mli_paged_attention_lean_gqa) held to
fp32 rounding error against the float64 model on the expanded operands (tests/gqa_model.py; tests/test_gqa_model_cpu.py
proves that the comparison bites), and to the BITS of mli_decode_scan_paged_sinks with n_heads heads on the expanded pages.

  B, S, D         H / Hkv (g)                 pages       forms (W, K)                what it reaches
  40, 64, 64      2/1 (2)                     f32, bf16   plain, (17,0), (16,4)       one item per row, 8- and 4-lane groups, dead lanes
  24, 256, 512    8/4 (2) 8/2 (4) 8/1 (8)     f32, bf16   plain, (100,20), (40,0)     f32: two lane loads, the two units of a lane in
                  2/1 (2)                                                             different groups; items of 256 and 1024 tokens
  24, 256, 192    3/1 (3) 6/2 (3)             f32, bf16   plain, (100,4)              g = 3, a width that leaves lanes dead
  20, 1024, 256   8/2 (4) 2/1 (2)             f32, bf16   (100,0), (256,0), plain,    many items per row, windows, sinks
                                                          (513,4)
  24, 512, 1024   8/2 (4)                     bf16        plain, (130,4)              bf16 two lane loads; items of 256 and 1024
  16, 4096, 512   4/1 (4)                     bf16        plain, (1024,0)             items of 64 and 1024 tokens: 64 items per row and 4
  700, 128, 64    2/1 (2)                     f32         plain, (50,4)               rows handed out longest first; grid order too

Lengths: accuracy_cases.edge_lengths with the form's W and K + W among the forced edges; 0 and S - 1 are asserted.  Poison:
after the conversion to the page type NaN is written into the K and V slots >= L and, under a window, into the gap slots
[K, lo); the page-table entries of the pages wholly inside the gap point at a NaN page, and once are null (same bits).  The
columns >= Dkv of K and V hold random values first and NaN afterwards: same bits, which is the test of "the scan reads Dkv
columns".  Tolerance: the project's rule (f64_model.tolerance) per score family, the family of a query head being its K/V
head's.  For bf16 pages the model is evaluated on the rounded pool."""
import functools
from types import SimpleNamespace

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
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

# base case outermost, so that the cached base (and its lengths) serves its page types and assignments in a row
CASES = [(seed, B, S, D, H, Hkv, W, K, elem, chunks, assignment)
         for seed, B, S, D, heads, elems, chunks in gm.GQA_SHAPES for H, Hkv, forms in heads for W, K in forms
         for elem in elems for assignment in hm.ASSIGNMENTS]


def _lengths(seed, B, S, W, K, chunks):
    if W == 0:
        return edge_lengths(seed, B, S, chunks)
    return edge_lengths(seed, B, S, (64, W) + ((K + W,) if K else ()))


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, W, K, chunks):
    return base_case(seed, B, S, D, _lengths(seed, B, S, W, K, chunks))


@functools.lru_cache(maxsize=1)
def _base_with(seed, B, S, D, lengths):
    return base_case(seed, B, S, D, np.asarray(lengths, np.int32))


def _unread_offsets(c, D, Dkv):
    """Pool offsets (in elements) of the K and V columns >= Dkv of every slot of every page a row owns"""
    pages = c["table"][c["table"] >= 0].astype(np.int64)
    slot = (np.arange(16) * 3 * D)[None, :, None]
    seg = np.concatenate([D + np.arange(Dkv, D), 2 * D + np.arange(Dkv, D)])[None, None, :]
    return (pages[:, None, None] + slot + seg).reshape(-1)


def _device_tables(c, pool, elem, W, K, nan_page, dev):
    """(all entries valid, the entries of the pages wholly inside the gap -> the NaN page, ... -> null)"""
    full = np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64)
    if W == 0:
        return _t(full, dev), _t(full, dev), _t(full, dev)
    gap = sm.gap_pages(c["lengths"], full.shape[1], W, K)
    return _t(full, dev), _t(np.where(gap, nan_page.data_ptr(), full), dev), _t(np.where(gap, 0, full), dev)


def _inputs(oracle, dev, c, H, Hkv, W, K, assignment, elem):
    """x.pool / x.table*: the grouped pages (K / V blocks 0 .. Hkv - 1 meaningful); x.xpool / x.xtable: the expanded pages, on
    which the H-head scan with sinks is the reference for the bits.  Model and oracle: on what the expanded pool holds."""
    q, kt = gm.apply_gqa_families(c, H, Hkv, assignment)
    B, D, S = kt.shape
    L, v = c["lengths"], c["v_cache"]
    pool32, off = fill_pages(oracle, c, q, kt, v)
    xpool32, xoff = fill_pages(oracle, c, q, gm.expand_kv(kt, H, Hkv, 1), gm.expand_kv(v, H, Hkv, 2))
    assert np.array_equal(off, xoff)
    gap = sm.gap_offsets(c["table"], L, S, D, W, K) if W else np.zeros(0, np.int64)
    dead = np.concatenate([off, gap])
    pool, _ = _poisoned_pool(pool32, dead, elem, dev)
    xpool, values = _poisoned_pool(xpool32, dead, elem, dev)
    s_live = max(-(-int(L.max()) // 16) * 16, 16)
    ktm = fm.gather_pages(values, c["table"], L, s_live, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, s_live, D, 2)
    nan_page = _nan_page(D, elem, dev)
    full, to_nan, to_null = _device_tables(c, pool, elem, W, K, nan_page, dev)
    xfull, x_nan, _ = _device_tables(c, xpool, elem, W, K, nan_page, dev)
    Wm = W if W else s_live          # the models' "no window": a window of the whole row
    return SimpleNamespace(q=_t(q, dev), L=_t(L, dev), table=full, table_nan=to_nan, table_null=to_null, pool=pool, xpool=xpool,
                           xtable=xfull, xtable_nan=x_nan, nan_page=nan_page, B=B, S=S, D=D, H=H, Hkv=Hkv, W=W, K=K, lengths=L,
                           unread=_unread_offsets(c, D, D // H * Hkv), fams=gm.head_families(assignment, H, Hkv),
                           model=sm.model_sinks(q, ktm, v_rows, L, H, Wm, K),
                           oracle=sm.oracle_sinks(oracle, q, ktm, v_rows, L, H, Wm, K))


def _poison_unread_columns(x, elem):
    offs = _t(x.unread, x.q.device)
    if elem == "f32":
        x.pool[offs] = float("nan")
    else:
        x.pool.view(torch.int16)[offs] = 0x7FC0


def _gqa(ops, x, elem, table=None, n_kv_heads=None, q=None):
    out = torch.full((x.B, x.D), SENTINEL, device=x.q.device)
    ops.decode_scan_paged_gqa(x.q if q is None else q, x.table_nan if table is None else table, x.L, out, x.H,
                              x.Hkv if n_kv_heads is None else n_kv_heads, x.W, x.K, ELEM[elem], x.S)
    return host(out).copy()


def _sinks_on_expanded_pages(ops, x, elem, table=None):
    """mli_decode_scan_paged_sinks with H heads (no window: a window of n_sequence there)"""
    out = torch.full((x.B, x.D), SENTINEL, device=x.q.device)
    ops.decode_scan_paged_sinks(x.q, x.xtable_nan if table is None else table, x.L, out, x.H, x.W if x.W else x.S, x.K, ELEM[elem],
                                x.S)
    return host(out).copy()


def _counters_are_zero(ops, x):
    ws, need = ops.workspace_for(x.B, x.S, x.D, x.q.device, x.H)
    assert need > 65536 and not host(ws[:65536]).any(), "the arrival counters are zero between calls"


def _forced_items(S, D, elem):
    """0 = the heuristic's item size.  Rows of two lane loads (fp32 D 512, bf16 D 1024) also run items of 256 and 1024 tokens, so
    that a wave owns several pages and its prefetch rolls across page boundaries; the long rows run 64 items per row and 4."""
    if S == 4096:
        return (64, 1024)
    return (0, 256, 1024) if D // (4 if elem == "f32" else 8) > 64 else (0,)


@pytest.mark.parametrize("seed,B,S,D,H,Hkv,W,K,elem,chunks,assignment", CASES)
def test_gqa_scan(oracle, mli, dev, seed, B, S, D, H, Hkv, W, K, elem, chunks, assignment):
    from min_llm_inference_amd import ops
    x = _inputs(oracle, dev, _base(seed, B, S, D, W, K, chunks), H, Hkv, W, K, assignment, elem)
    assert x.lengths.min() == 0 and x.lengths.max() == S - 1 and Hkv < H and (W == 0 or K + W < S)
    results, first = [], {}
    try:
        for ct in _forced_items(S, D, elem):
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            what = f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} K{K} {elem} chunk_tokens {ct}"
            got = first[ct] = _gqa(ops, x, elem)
            results += gm.compare(got, x.oracle, x.model, x.fams, what=what)
            assert_equal(got, _sinks_on_expanded_pages(ops, x, elem),
                         what=f"{what}: the scan with sinks at {H} heads on the expanded pages")
            assert_equal(_gqa(ops, x, elem), got, what=f"{what}: second launch (deterministic merge, counters back at zero)")
            _counters_are_zero(ops, x)
            if W:
                assert_equal(_gqa(ops, x, elem, table=x.table_null), got,
                             what=f"{what}: null page-table entries inside the gap against entries of a NaN page")
            for nt in (0, 1):                            # both cache policies of the K / V loads
                assert mli.mli_tune(b"nt_loads", nt) == 0
                assert_equal(_gqa(ops, x, elem), got, what=f"{what} nt_loads {nt}")
            mli.mli_tune(b"nt_loads", 2)
            if B > 512:                                  # one item per row, longest first by default: grid order too
                assert mli.mli_tune(b"scan_row_order", 0) == 0
                assert_equal(_gqa(ops, x, elem), got, what=f"{what} grid order")
                mli.mli_tune(b"scan_row_order", 1)
        # the grouping is not a no-op: n_heads heads on the same (grouped) pages read the columns >= Dkv and give something else
        ct0 = _forced_items(S, D, elem)[0]
        assert mli.mli_tune(b"chunk_tokens", ct0) == 0
        ungrouped = _gqa(ops, x, elem, n_kv_heads=H)
        assert np.isfinite(ungrouped).all() and np.abs(ungrouped - first[ct0]).max() > 1e-3, "n_kv_heads changes nothing"
        # the K and V columns >= Dkv of every slot are never read: NaN there changes no bit
        _poison_unread_columns(x, elem)
        for ct in _forced_items(S, D, elem):
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            what = f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} K{K} {elem} chunk_tokens {ct}, NaN in the columns >= Dkv"
            got = _gqa(ops, x, elem)
            assert np.isfinite(got).all() and (got != SENTINEL).all(), what
            results += gm.compare(got, x.oracle, x.model, x.fams, what=what)
            assert_equal(got, first[ct], what=what)
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
        mli.mli_tune(b"nt_loads", 2)
        mli.mli_tune(b"scan_row_order", 1)
    gm.assert_within(results, f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} K{K} {elem}")


@pytest.mark.parametrize("H,Hkv,W,K,elem", [(2, 1, 0, 0, "f32"), (8, 2, 256, 4, "bf16"), (8, 4, 100, 0, "f32")])
def test_gqa_scan_with_rows_of_S_tokens(oracle, mli, dev, H, Hkv, W, K, elem):
    """The S = 1024 shape with its two long random rows made full: L == n_sequence, all S / 16 pages present (the scan clamps
    with min(L, S); every other case stops at S - 1); a row of length 0 beside them."""
    from min_llm_inference_amd import ops
    seed, B, S, D = 304, 20, 1024, 256
    L = _lengths(seed, B, S, W, K, (64, 256))
    rows = np.nonzero((L >= 3 * S // 4) & (L < S - 2))[0][:2]
    assert len(rows) == 2
    L[rows] = S
    x = _inputs(oracle, dev, _base_with(seed, B, S, D, tuple(L.tolist())), H, Hkv, W, K, "mixed", elem)
    assert x.lengths.min() == 0 and x.lengths.max() == S and (x.lengths == S).sum() == 2
    what = f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} K{K} {elem}, rows of S tokens"
    got = _gqa(ops, x, elem)
    assert (got[x.lengths == 0] == 0).all()
    results = gm.compare(got, x.oracle, x.model, x.fams, what=what)
    assert_equal(got, _sinks_on_expanded_pages(ops, x, elem), what=f"{what}: the scan with sinks on the expanded pages")
    assert_equal(_gqa(ops, x, elem), got, what=f"{what}: second launch")
    _counters_are_zero(ops, x)
    gm.assert_within(results, what)


@pytest.mark.parametrize("H,W,K,elem", [(1, 0, 0, "f32"), (1, 100, 20, "bf16"), (8, 0, 0, "f32"), (8, 100, 20, "bf16"),
                                        (8, 40, 0, "f32"), (2, 100, 156, "bf16")])
def test_equal_head_counts_are_the_scan_with_sinks_bit_for_bit(oracle, mli, dev, H, W, K, elem):
    """n_kv_heads == n_heads is mli_decode_scan_paged_sinks on the same pages: same kernels, same bits, one head included"""
    from min_llm_inference_amd import ops
    seed, B, S, D = 302, 24, 256, 512
    c = _base(seed, B, S, D, W, K, (64, 256))
    x = _inputs(oracle, dev, c, H, H, W, K, "flat", elem)
    x.xtable_nan = x.table_nan                 # the reference runs on the same pages
    want = _sinks_on_expanded_pages(ops, x, elem)
    assert np.isfinite(want).all() and (want != SENTINEL).all()
    assert_equal(_gqa(ops, x, elem), want, what=f"H{H} = Hkv W{W} K{K} {elem}")


def test_a_plain_call_of_another_shape_shares_the_buffer(oracle, mli, dev):
    """One workspace serves both kinds of call: a plain scan, a grouped-query scan of a different shape in the same buffer, the
    plain scan again -- same bits as before, and the grouped-query result still within tolerance."""
    from min_llm_inference_amd import ops
    y = _inputs(oracle, dev, _base(304, 20, 1024, 256, 0, 0, (64, 256)), 8, 2, 0, 0, "mixed", "f32")
    x = _inputs(oracle, dev, _base(302, 24, 256, 512, 0, 0, (64, 256)), 8, 8, 0, 0, "flat", "f32")
    big, _ = ops.workspace_for(y.B, y.S, y.D, dev, y.H)          # grown once, for the larger need

    def plain():
        out = torch.full((x.B, x.D), SENTINEL, device=dev)
        ops.decode_scan_paged(x.q, x.table, x.L, None, out, 0, phases=7, n_sequence=x.S)
        assert ops.workspace_for(x.B, x.S, x.D, dev)[0].data_ptr() == big.data_ptr(), "the calls share one buffer"
        return host(out).copy().view(np.uint32)   # bit patterns: one head over the whole width reads the NaN of the dead slots

    before = plain()
    got = _gqa(ops, y, "f32")
    assert ops.workspace_for(y.B, y.S, y.D, dev, y.H)[0].data_ptr() == big.data_ptr()
    assert_equal(plain(), before, what="plain scan after a grouped-query scan in the same workspace")
    gm.assert_within(gm.compare(got, y.oracle, y.model, y.fams, what="grouped-query scan between two plain scans"))
    gm.assert_within(gm.compare(_gqa(ops, y, "f32"), y.oracle, y.model, y.fams, what="grouped-query scan after a plain scan"))
    assert_equal(plain(), before, what="plain scan after the second grouped-query scan")


@pytest.mark.parametrize("elem,W,K", [("f32", None, None), ("bf16", 40, 4)])
def test_lean_gqa_composition(oracle, mli, dev, elem, W, K):
    """mli_paged_attention_lean_gqa with new rows: pages and q_output bit-identical to mli_paged_attention_lean on the same
    inputs (fill and projection are the existing launches and do not depend on n_kv_heads), attention_result against the
    model on the expansion of what the call left in memory (q_output and the pages, the appended K / V rows included)."""
    from accuracy_cases import dead_slot_offsets
    from helpers import paged_case
    from min_llm_inference_amd import ops
    seed, B, S, D, H, Hkv = 621, 20, 256, 256, 4, 2
    L = edge_lengths(seed, B, S, (64, 44))
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    new = [int(np.nonzero(L == n)[0][0]) for n in (2, 17, 45, 65)]
    c["n_new"] = len(new)
    c["new_batch_idx"][:len(new)] = new
    pool32 = c["pool"].copy()
    oracle.clone_to_pages(pool32, c["table"], c["inp_embedding"], c["kt_cache"], c["v_cache"], L)
    off, _, _ = dead_slot_offsets(c["table"], L, S, D)
    wdt = torch.float32 if elem == "f32" else torch.bfloat16

    def run(n_heads, n_kv_heads):
        pool, _ = _poisoned_pool(pool32, off, elem, dev)
        d = SimpleNamespace(pool=pool, q=_t(c["q_output"], dev), out=torch.full((B, D), SENTINEL, device=dev))
        table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
        w = [_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv")]
        ops.paged_attention_lean(table, _t(L, dev), w[0], w[1], w[2], _t(c["new_batch_idx"], dev), d.q, d.out, c["n_new"], S,
                                 elem=ELEM[elem], n_heads=n_heads, window=W, sinks=K, n_kv_heads=n_kv_heads)
        torch.cuda.synchronize()
        return d

    one, many, grouped, same = run(1, None), run(H, None), run(H, Hkv), run(H, H)
    bits = torch.int32 if elem == "f32" else torch.int16
    assert torch.equal(one.pool.view(bits), grouped.pool.view(bits)), "pages do not depend on n_kv_heads"
    assert_equal(host(grouped.q), host(one.q), what="q_output does not depend on n_kv_heads")
    assert_equal(host(same.out), host(many.out), what="n_kv_heads == n_heads is the call without it")
    values = torch.nan_to_num(grouped.pool.float()).cpu().numpy()
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q = host(grouped.q)
    model = gm.model_gqa(q, ktm, v_rows, L, H, Hkv, W or 0, K or 0)
    res = gm.compare(host(grouped.out), gm.oracle_gqa(oracle, q, ktm, v_rows, L, H, Hkv, W or 0, K or 0), model, ("flat",) * H,
                     what=f"lean grouped-query composition {elem}")
    gm.assert_within(res, f"mli_paged_attention_lean_gqa {elem}")
    assert not np.array_equal(host(grouped.out), host(many.out)), "two K/V heads give what four give"
