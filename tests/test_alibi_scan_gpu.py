"""The multi-head paged scan with ALiBi (mli_decode_scan_paged_alibi, mli_paged_attention_lean_alibi) held to fp32 rounding error
against the float64 model with the bias (tests/alibi_model.py; tests/test_alibi_model_cpu.py proves that the comparison bites),
on fp32 and bf16 pages; for bf16 pages the model is evaluated on the rounded pool.

  B, S, D, H          pages       what it reaches
  5, 64, 128, 4       f32, bf16   one item per row
  6, 1024, 256, 8     f32, bf16   chunk_tokens 0, 64 and 256: several items per row, the bias frame across items
  4, 256, 512, 8      f32         two lane loads: the two units of a lane carry the slopes of different heads
  4, 256, 1024, 16    bf16        ... on bf16 pages
  4, 128, 192, 3      f32, bf16   dead lanes, a head count that is no power of two
  600, 64, 64, 2      f32         rows handed out longest first

each with n_kv_heads in {H, a proper divisor, 1} and (W, K) in {none, (40, 0), (5, 0), (40, 4), (40, 20)}.  Lengths: 0, 1, 16,
17 and S in every case (dealt over several length vectors where the batch has fewer rows), S - 1, and random rows.  Judged by
  - the model under the tolerance derived from its float32 evaluation, with the standard slopes, all negative ones and mixed ones;
  - slopes all 0.0f: the bits of mli_decode_scan_paged_gqa on the same pages;
  - L == 1, and a one-slot window: V's row L - 1 bit for bit, whatever the slopes;
  - NaN in the dead slots, the gap slots and behind the page-table entries of the gap pages (and null entries there): the bits
    the clean pages give;
  - a second launch: the same bits; the arrival counters back at zero;
  - one workspace: a plain scan, an ALiBi scan of another shape in the same buffer, the plain scan again."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import alibi_model as am
import f64_model as fm
import gqa_model as gm
import sinks_model as sm
from accuracy_cases import base_case, fill_pages
from gpu_util import host
from helpers import assert_equal
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

FORMS = ((0, 0), (40, 0), (5, 0), (40, 4), (40, 20))
# (seed, B, S, D, H, page types, n_kv_heads, chunk_tokens)
SHAPES = [
    (711, 5, 64, 128, 4, ("f32", "bf16"), (4, 2, 1), (0,)),
    (712, 6, 1024, 256, 8, ("f32", "bf16"), (8, 2, 1), (0, 64, 256)),
    (713, 4, 256, 512, 8, ("f32",), (8, 4, 1), (0,)),
    (714, 4, 256, 1024, 16, ("bf16",), (16, 4, 1), (0,)),
    (715, 4, 128, 192, 3, ("f32", "bf16"), (3, 1), (0,)),
    (716, 600, 64, 64, 2, ("f32",), (2, 1), (0,)),
]
CASES = [(seed, B, S, D, H, elem, Hkv, chunks) for seed, B, S, D, H, elems, kvs, chunks in SHAPES for elem in elems for Hkv in kvs]


def length_vectors(seed, B, S):
    """Length vectors of B rows that together hold 0, 1, 16, 17, S, S - 1, a row one token into its last page and random rows in
    the upper half (rows with a gap under every window of FORMS)."""
    rng = np.random.default_rng(seed + 9400)
    want = [0, 1, 16, 17, S, S - 1, S - 15]
    n = -(-len(want) // B) if B < len(want) + 2 else 1
    parts = []
    for i in range(n):
        share = want[i::n]
        share += rng.integers(S // 2, S + 1, size=B - len(share)).tolist()
        parts.append(np.asarray(share, np.int32))
    assert set(np.concatenate(parts).tolist()) >= set(want)
    return parts


@functools.lru_cache(maxsize=2)
def _pages(seed, B, S, D, elem, part):
    """The case's pages in `elem` and the values they hold, once per (shape, page type, length vector)"""
    import oracle
    oracle.lib()
    L = length_vectors(seed, B, S)[part]
    c = base_case(seed, B, S, D, L)
    pool32, dead = fill_pages(oracle, c, c["q_output"], c["kt_cache"], c["v_cache"])
    dev = torch.device("cuda:0")
    clean, values = _poisoned_pool(pool32, np.zeros(0, np.int64), elem, dev)
    s_live = max(-(-int(L.max()) // 16) * 16, 16)
    return SimpleNamespace(c=c, L=L, B=B, S=S, D=D, elem=elem, pool32=pool32, dead=dead, clean=clean, q=c["q_output"],
                           kt=fm.gather_pages(values, c["table"], L, s_live, D, 1).transpose(0, 2, 1),
                           v=fm.gather_pages(values, c["table"], L, s_live, D, 2), dq=_t(c["q_output"], dev), dL=_t(L, dev),
                           nan_page=_nan_page(D, elem, dev),
                           table=_t(np.where(c["table"] >= 0, clean.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev))


def _poisoned(x, W, K):
    """(pool with NaN in the dead and the gap slots, table whose gap pages are the NaN page, table whose gap pages are null)"""
    dev = x.dq.device
    gap = sm.gap_offsets(x.c["table"], x.L, x.S, x.D, W, K) if W else np.zeros(0, np.int64)
    pool, _ = _poisoned_pool(x.pool32, np.concatenate([x.dead, gap]), x.elem, dev)
    full = np.where(x.c["table"] >= 0, pool.data_ptr() + ESIZE[x.elem] * x.c["table"], 0).astype(np.int64)
    if not W:
        return pool, _t(full, dev), _t(full, dev)
    gp = sm.gap_pages(x.L, full.shape[1], W, K)
    return pool, _t(np.where(gp, x.nan_page.data_ptr(), full), dev), _t(np.where(gp, 0, full), dev)


def _alibi(ops, x, table, H, Hkv, W, K, slopes):
    out = torch.full((x.B, x.D), SENTINEL, device=x.dq.device)
    ops.decode_scan_paged_alibi(x.dq, table, x.dL, out, H, Hkv, W, K, _t(np.asarray(slopes, np.float32), x.dq.device), ELEM[x.elem], x.S)
    return host(out).copy()


def _gqa(ops, x, table, H, Hkv, W, K):
    out = torch.full((x.B, x.D), SENTINEL, device=x.dq.device)
    ops.decode_scan_paged_gqa(x.dq, table, x.dL, out, H, Hkv, W, K, ELEM[x.elem], x.S)
    return host(out).copy()


def _counters_are_zero(ops, x, H):
    ws, need = ops.workspace_for(x.B, x.S, x.D, x.dq.device, H)
    assert need > 65536 and not host(ws[:65536]).any(), "the arrival counters are zero between calls"


def _newest_v_rows(x, H, Hkv):
    """[B, D]: row b = V's row L - 1 as query head h reads it (block h // g), zeros for L == 0"""
    want = np.zeros((x.B, x.D), np.float32)
    v = gm.expand_kv(x.v, H, Hkv, 2)
    for b in np.nonzero(x.L > 0)[0]:
        want[b] = v[b, x.L[b] - 1]
    return want


@pytest.mark.parametrize("seed,B,S,D,H,elem,Hkv,chunks", CASES)
def test_alibi_scan(mli, dev, seed, B, S, D, H, elem, Hkv, chunks):
    from min_llm_inference_amd import ops
    sets = am.slope_sets(H, seed)
    failures = []
    launches = 0
    assert mli.mli_launch_counts_reset() == 0
    try:
        for part in range(len(length_vectors(seed, B, S))):
            x = _pages(seed, B, S, D, elem, part)
            for W, K in FORMS:
                assert W == 0 or K + W < S
                pool, table_nan, table_null = _poisoned(x, W, K)
                models = {name: am.AlibiModel(x.q, x.kt, x.v, x.L, H, Hkv, m, W, K) for name, m in sets.items()}
                o32 = {name: am.eval_fp32(x.q, x.kt, x.v, x.L, H, Hkv, m, W, K) for name, m in sets.items()}
                ones = x.L == 1
                for ct in chunks:
                    assert mli.mli_tune(b"chunk_tokens", ct) == 0
                    what = f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} K{K} {elem} part {part} chunk_tokens {ct}"
                    for name, m in sets.items():
                        got = _alibi(ops, x, table_nan, H, Hkv, W, K, m)
                        launches += 1
                        assert (got[x.L == 0] == 0).all(), f"{what} {name}: rows of length 0"
                        worst, tol = am.compare(got, o32[name], models[name], what=f"{what} | {name}")
                        if not worst <= tol:
                            failures.append(f"{what} [{name}]: {worst:.3e} > tol {tol:.3e}")
                        assert_equal(got[ones], _newest_v_rows(x, H, Hkv)[ones], what=f"{what} {name}: L == 1 is V's row 0")
                        if name != "standard":
                            continue
                        assert_equal(_alibi(ops, x, table_nan, H, Hkv, W, K, m), got, what=f"{what}: second launch")
                        _counters_are_zero(ops, x, H)
                        assert_equal(_alibi(ops, x, x.table, H, Hkv, W, K, m), got, what=f"{what}: clean pages against NaN in the "
                                     "dead slots, the gap slots and the gap pages")
                        launches += 2
                        if W:
                            assert_equal(_alibi(ops, x, table_null, H, Hkv, W, K, m), got, what=f"{what}: null entries in the gap")
                            launches += 1
                        if not (sets["standard"] == 0).all() and (x.L > 17).any():
                            plain = _gqa(ops, x, table_nan, H, Hkv, W, K)
                            assert np.abs(plain - got).max() > 1e-3, f"{what}: the slopes change nothing"
                    zero = _alibi(ops, x, table_nan, H, Hkv, W, K, np.zeros(H, np.float32))
                    launches += 1
                    assert_equal(zero, _gqa(ops, x, table_nan, H, Hkv, W, K), what=f"{what}: slopes all zero against the _gqa call")
                del pool
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
    assert ops.launch_count("scan_heads_alibi") == launches
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("seed,B,S,D,H,elem,Hkv", [(711, 5, 64, 128, 4, "f32", 2), (712, 6, 1024, 256, 8, "bf16", 8),
                                                   (714, 4, 256, 1024, 16, "bf16", 4), (713, 4, 256, 512, 8, "f32", 1)])
def test_a_one_slot_window_gives_the_newest_v_row_bit_for_bit(mli, dev, seed, B, S, D, H, elem, Hkv):
    from min_llm_inference_amd import ops
    for part in range(len(length_vectors(seed, B, S))):
        x = _pages(seed, B, S, D, elem, part)
        pool, table_nan, _ = _poisoned(x, 1, 0)
        for name, m in am.slope_sets(H, seed).items():
            got = _alibi(ops, x, table_nan, H, Hkv, 1, 0, m)
            assert_equal(got, _newest_v_rows(x, H, Hkv), what=f"B{B} S{S} D{D} H{H} Hkv{Hkv} {elem} W 1 {name}")
        del pool


def test_a_plain_call_of_another_shape_shares_the_buffer(mli, dev):
    """One workspace serves both kinds of call: a plain scan, an ALiBi scan of a different shape in the same buffer, the plain
    scan again -- same bits as before, and the ALiBi result within tolerance both times."""
    from min_llm_inference_amd import ops
    y = _pages(712, 6, 1024, 256, "f32", 0)
    H, Hkv = 8, 2
    big, _ = ops.workspace_for(y.B, y.S, y.D, dev, H)          # grown once, for the larger need
    x = _pages(711, 5, 64, 128, "f32", 0)
    m = am.standard_slopes(H)
    model, o32 = am.AlibiModel(y.q, y.kt, y.v, y.L, H, Hkv, m), am.eval_fp32(y.q, y.kt, y.v, y.L, H, Hkv, m)

    def plain():
        out = torch.full((x.B, x.D), SENTINEL, device=dev)
        ops.decode_scan_paged(x.dq, x.table, x.dL, None, out, 0, phases=7, n_sequence=x.S)
        assert ops.workspace_for(x.B, x.S, x.D, dev)[0].data_ptr() == big.data_ptr(), "the calls share one buffer"
        return host(out).copy().view(np.uint32)

    before = plain()
    for what in ("between two plain scans", "after a plain scan"):
        got = _alibi(ops, y, y.table, H, Hkv, 0, 0, m)
        assert ops.workspace_for(y.B, y.S, y.D, dev, H)[0].data_ptr() == big.data_ptr()
        worst, tol = am.compare(got, o32, model, what=f"ALiBi scan {what}")
        assert worst <= tol
        assert_equal(plain(), before, what=f"plain scan after the ALiBi scan ({what})")


@pytest.mark.parametrize("elem,W,K", [("f32", None, None), ("bf16", 40, 4)])
def test_lean_alibi_composition(oracle, mli, dev, elem, W, K):
    """mli_paged_attention_lean_alibi with new rows: pages and q_output bit-identical to mli_paged_attention_lean_gqa on the same
    inputs (fill and projection never see the slopes), attention_result against the model on what the call left in memory."""
    from accuracy_cases import dead_slot_offsets, edge_lengths
    from helpers import paged_case
    from min_llm_inference_amd import ops
    seed, B, S, D, H, Hkv = 721, 20, 256, 256, 4, 2
    L = edge_lengths(seed, B, S, (64, 44))
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    new = [int(np.nonzero(L == n)[0][0]) for n in (2, 17, 45, 65)]
    c["n_new"] = len(new)
    c["new_batch_idx"][:len(new)] = new
    pool32 = c["pool"].copy()
    oracle.clone_to_pages(pool32, c["table"], c["inp_embedding"], c["kt_cache"], c["v_cache"], L)
    off, _, _ = dead_slot_offsets(c["table"], L, S, D)
    wdt = torch.float32 if elem == "f32" else torch.bfloat16
    slopes = am.standard_slopes(H)

    def run(alibi):
        pool, _ = _poisoned_pool(pool32, off, elem, dev)
        d = SimpleNamespace(pool=pool, q=_t(c["q_output"], dev), out=torch.full((B, D), SENTINEL, device=dev))
        table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
        w = [_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv")]
        ops.paged_attention_lean(table, _t(L, dev), w[0], w[1], w[2], _t(c["new_batch_idx"], dev), d.q, d.out, c["n_new"], S,
                                 elem=ELEM[elem], n_heads=H, window=W, sinks=K, n_kv_heads=Hkv,
                                 alibi_slopes=_t(slopes, dev) if alibi else None)
        torch.cuda.synchronize()
        return d

    plain, biased = run(False), run(True)
    bits = torch.int32 if elem == "f32" else torch.int16
    assert torch.equal(plain.pool.view(bits), biased.pool.view(bits)), "pages do not depend on the slopes"
    assert_equal(host(biased.q), host(plain.q), what="q_output does not depend on the slopes")
    values = torch.nan_to_num(biased.pool.float()).cpu().numpy()
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q = host(biased.q)
    model = am.AlibiModel(q, ktm, v_rows, L, H, Hkv, slopes, W or 0, K or 0)
    worst, tol = am.compare(host(biased.out), am.eval_fp32(q, ktm, v_rows, L, H, Hkv, slopes, W or 0, K or 0), model,
                            what=f"lean ALiBi composition {elem}")
    assert worst <= tol
    assert np.abs(host(biased.out) - host(plain.out)).max() > 1e-3, "the slopes change nothing"
