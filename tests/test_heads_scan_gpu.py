"""The multi-head paged scan (mli_decode_scan_paged_heads, mli_paged_attention_lean_heads) held to fp32 rounding error
against the per-head float64 model (tests/heads_model.py; tests/test_heads_model_cpu.py proves that the comparison
bites).  Shapes: the smallest at which each mechanism can still go wrong --

  B, S, D         H (head_dim)      pages       what it reaches
  40, 64, 64      2 (32)            f32, bf16   one item per row, 8- and 4-lane groups, dead lanes
  24, 256, 512    8 (64), 2 (256)   f32, bf16   several chunks, per-head merge in the kernel; f32: two lane loads, one head per
                                                load at 256; chunk_tokens 256: several pages per wave
  24, 256, 192    3 (64)            f32, bf16   a width that leaves lanes dead, odd head count
  20, 1024, 256   2 (128), 8 (32)   f32, bf16   16 chunks per row
  24, 512, 1024   8 (128)           bf16        two lane loads, bf16; chunk_tokens 256 / 1024: several pages per wave
  16, 4096, 512   4 (128)           bf16        chunk_tokens 64 and 1024: 64 items per row and 4
  700, 128, 64    2 (32)            f32         rows handed out longest first (B > 512, one item per row)

Lengths: accuracy_cases.edge_lengths (0, 1, 2, 15, 16, 17, chunk +- 1, S - 2, S - 1, two rows >= 3/4 S).  Dead slots of
K and V are NaN, written after the conversion to the page type; for bf16 the model is evaluated on the bf16-rounded pool,
read back through gather_pages.  Tolerance: max(8 x the per-head oracle's error, 16 x 2^-24), per score family."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import f64_model as fm
import heads_model as hm
from accuracy_cases import base_case, dead_slot_offsets, edge_lengths, fill_pages
from gpu_util import host
from helpers import assert_equal, paged_case

pytestmark = pytest.mark.gpu

SENTINEL = 12345.0
ELEM = {"f32": 0, "bf16": 1}
ESIZE = {"f32": 4, "bf16": 2}
CASES = [(seed, B, S, D, H, elem, chunks) for seed, B, S, D, heads, elems, chunks in hm.HEAD_SHAPES for H in heads
         for elem in elems]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, chunks):
    return base_case(seed, B, S, D, edge_lengths(seed, B, S, chunks))


@functools.lru_cache(maxsize=1)
def _base_with(seed, B, S, D, lengths):
    return base_case(seed, B, S, D, np.asarray(lengths, np.int32))


def _poisoned_pool(pool32, off, elem, dev):
    """(device pool of the page type with NaN in the dead K / V slots, the float32 values the live slots hold)"""
    t = _t(pool32, dev)
    offs = _t(off, dev) if len(off) else None
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


def _inputs(oracle, dev, c, H, assignment, elem):
    q, kt = hm.apply_head_families(c, H, assignment)
    B, D, S = kt.shape
    L = c["lengths"]
    pool32, off = fill_pages(oracle, c, q, kt, c["v_cache"])
    pool, values = _poisoned_pool(pool32, off, elem, dev)
    s_live = max(-(-int(L.max()) // 16) * 16, 16)
    ktm = fm.gather_pages(values, c["table"], L, s_live, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, s_live, D, 2)
    table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
    return SimpleNamespace(q=_t(q, dev), L=_t(L, dev), page_table=table, pool=pool, B=B, S=S, D=D, H=H, lengths=L,
                           model=hm.HeadsModel(q, ktm, v_rows, L, H), oracle=hm.oracle_heads(oracle, q, ktm, v_rows, L, H))


def _scan(ops, x, elem, n_heads=None):
    out = torch.full((x.B, x.D), SENTINEL, device=x.q.device)
    ops.decode_scan_paged_heads(x.q, x.page_table, x.L, out, x.H if n_heads is None else n_heads, ELEM[elem], x.S)
    return host(out).copy()


def _counters_are_zero(ops, x, n_heads):
    ws, need = ops.workspace_for(x.B, x.S, x.D, x.q.device, n_heads)
    assert need > 65536 and not host(ws[:65536]).any(), "the arrival counters are zero between calls"


@pytest.mark.parametrize("assignment", hm.ASSIGNMENTS)
@pytest.mark.parametrize("seed,B,S,D,H,elem,chunks", CASES)
def test_heads_scan(oracle, mli, dev, seed, B, S, D, H, elem, chunks, assignment):
    from min_llm_inference_amd import ops
    x = _inputs(oracle, dev, _base(seed, B, S, D, chunks), H, assignment, elem)
    assert x.lengths.min() == 0 and x.lengths.max() == S - 1
    # chunk_tokens 0 = the heuristic's item size (64 tokens at these batch sizes: one page per wave).  The long rows also
    # run 64 items per row and 4; the rows of two lane loads (fp32 D = 512, bf16 D = 1024) also run items of 256 tokens, and
    # the bf16 ones a single item of the whole row, so that a wave owns 4 and 8 pages and its prefetch rolls across page
    # boundaries in every kernel variant
    forced = (64, 1024) if S == 4096 else (0, 256, 1024) if D == 1024 else (0, 256) if D == 512 else (0,)
    results = []
    try:
        for ct in forced:
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            what = f"B{B} S{S} D{D} H{H} {elem} chunk_tokens {ct}"
            got = _scan(ops, x, elem)
            results += hm.compare(got, x.oracle, x.model, assignment, what=what)
            assert_equal(_scan(ops, x, elem), got, what=f"{what}: second launch (deterministic merge, counters back at zero)")
            _counters_are_zero(ops, x, H)
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
    hm.assert_within(results, f"B{B} S{S} D{D} H{H} {elem}")


@pytest.mark.parametrize("assignment", hm.ASSIGNMENTS)
@pytest.mark.parametrize("H,elem", [(2, "f32"), (8, "bf16")])
def test_heads_scan_with_rows_of_S_tokens(oracle, mli, dev, H, elem, assignment):
    """The S = 1024 shape with its two long random rows made full: L == n_sequence, all S / 16 pages present (the scan clamps
    with min(L, S); every other case stops at S - 1)."""
    from min_llm_inference_amd import ops
    seed, B, S, D, _, _, chunks = hm.HEAD_SHAPES[3]
    L = edge_lengths(seed, B, S, chunks)
    rows = np.nonzero((L >= 3 * S // 4) & (L < S - 2))[0][:2]
    assert len(rows) == 2
    L[rows] = S
    x = _inputs(oracle, dev, _base_with(seed, B, S, D, tuple(L.tolist())), H, assignment, elem)
    assert x.lengths.min() == 0 and x.lengths.max() == S and (x.lengths == S).sum() == 2
    what = f"B{B} S{S} D{D} H{H} {elem}, rows of S tokens"
    got = _scan(ops, x, elem)
    results = hm.compare(got, x.oracle, x.model, assignment, what=what)
    assert_equal(_scan(ops, x, elem), got, what=f"{what}: second launch")
    _counters_are_zero(ops, x, H)
    hm.assert_within(results, what)


@pytest.mark.parametrize("seed,B,S,D,elem", [(302, 24, 256, 512, "f32"), (304, 20, 1024, 256, "bf16")])
def test_one_head_is_todays_scan_bit_for_bit(oracle, mli, dev, seed, B, S, D, elem):
    from min_llm_inference_amd import ops
    x = _inputs(oracle, dev, _base(seed, B, S, D, (64, 256)), 1, "flat", elem)
    want = torch.full((B, D), SENTINEL, device=dev)
    ops.decode_scan_paged(x.q, x.page_table, x.L, None, want, ELEM[elem], phases=7, n_sequence=S)
    assert_equal(_scan(ops, x, elem, n_heads=1), host(want), what="n_heads 1 through mli_decode_scan_paged_heads")
    assert mli.mli_attention_heads_workspace_bytes(B, S, D, 1) == mli.mli_attention_workspace_bytes(B, S, D)


def test_a_single_head_call_of_another_shape_shares_the_buffer(oracle, mli, dev):
    """One workspace serves both kinds of call: a plain scan, a multi-head scan of a different shape in the same buffer,
    the plain scan again -- same bits as before, and the multi-head result still within tolerance."""
    from min_llm_inference_amd import ops
    y = _inputs(oracle, dev, _base(304, 20, 1024, 256, (64, 256)), 8, "mixed", "f32")
    x = _inputs(oracle, dev, _base(302, 24, 256, 512, (64, 256)), 1, "flat", "f32")
    big, _ = ops.workspace_for(y.B, y.S, y.D, dev, y.H)          # grown once, for the larger need

    def plain():
        out = torch.full((x.B, x.D), SENTINEL, device=dev)
        ops.decode_scan_paged(x.q, x.page_table, x.L, None, out, 0, phases=7, n_sequence=x.S)
        assert ops.workspace_for(x.B, x.S, x.D, dev)[0].data_ptr() == big.data_ptr(), "the calls share one buffer"
        return host(out).copy()

    before = plain()
    got = _scan(ops, y, "f32")
    assert ops.workspace_for(y.B, y.S, y.D, dev, y.H)[0].data_ptr() == big.data_ptr()
    assert_equal(plain(), before, what="plain scan after a multi-head scan in the same workspace")
    hm.assert_within(hm.compare(got, y.oracle, y.model, "mixed", what="multi-head scan between two plain scans"))
    hm.assert_within(hm.compare(_scan(ops, y, "f32"), y.oracle, y.model, "mixed", what="multi-head scan after a plain scan"))


@pytest.mark.parametrize("elem", ["f32", "bf16"])
def test_lean_heads_composition(oracle, mli, dev, elem):
    """mli_paged_attention_lean_heads with new rows: pages and q_output bit-identical to mli_paged_attention_lean on the same
    inputs (fill and projection are the existing launches), attention_result against the per-head model of what the call
    left in memory (q_output and the pages, the appended K / V rows included)."""
    from min_llm_inference_amd import ops
    seed, B, S, D, H = 321, 20, 256, 256, 4
    L = edge_lengths(seed, B, S, (64,))
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    new = [b for b in range(B) if int(L[b]) in (2, 17, 63, 65)]
    assert len(new) == 4
    c["n_new"] = len(new)
    c["new_batch_idx"][:len(new)] = new
    pool32 = c["pool"].copy()
    oracle.clone_to_pages(pool32, c["table"], c["inp_embedding"], c["kt_cache"], c["v_cache"], L)
    off, _, _ = dead_slot_offsets(c["table"], L, S, D)
    wdt = torch.float32 if elem == "f32" else torch.bfloat16

    def run(n_heads):
        pool, _ = _poisoned_pool(pool32, off, elem, dev)
        d = SimpleNamespace(pool=pool, q=_t(c["q_output"], dev), out=torch.full((B, D), SENTINEL, device=dev))
        table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
        w = [_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv")]
        ops.paged_attention_lean(table, _t(L, dev), w[0], w[1], w[2], _t(c["new_batch_idx"], dev), d.q, d.out, c["n_new"], S,
                                 elem=ELEM[elem], n_heads=n_heads)
        torch.cuda.synchronize()
        return d

    one, many = run(1), run(H)
    bits = torch.int32 if elem == "f32" else torch.int16
    assert torch.equal(one.pool.view(bits), many.pool.view(bits)), "pages do not depend on n_heads"
    assert_equal(host(many.q), host(one.q), what="q_output does not depend on n_heads")
    values = torch.nan_to_num(many.pool.float()).cpu().numpy()
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q = host(many.q)
    model = hm.HeadsModel(q, ktm, v_rows, L, H)
    res = hm.compare(host(many.out), hm.oracle_heads(oracle, q, ktm, v_rows, L, H), model, "flat", what=f"lean composition {elem}")
    hm.assert_within(res, f"mli_paged_attention_lean_heads {elem}")
    assert not np.array_equal(host(many.out), host(one.out)), "four heads give what one head gives"
