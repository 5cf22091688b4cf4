"""The multi-head paged scan with logit soft-capping (mli_decode_scan_paged_softcap, mli_paged_attention_lean_softcap) held to fp32
rounding error against the float64 model with the cap (tests/softcap_model.py; tests/test_softcap_model_cpu.py proves that the
comparison bites on inputs scaled as here), on fp32 and bf16 pages; for bf16 pages the model is evaluated on the rounded pool.

The shapes, n_kv_heads, forms and length vectors are those of tests/test_alibi_scan_gpu.py (its table says what each reaches):
one item per row; several items per row under chunk_tokens 0, 64 and 256; two lane loads on fp32 and on bf16 pages; dead lanes
and a head count that is no power of two; rows handed out longest first.  q is scaled so that the largest score of the case is
half the largest cap (softcap_model.scale_q): the condition under which a wrong cap is visible at every cap.  Caps 50, 5, 1.
Judged by
  - the model under the tolerance derived from its float32 evaluation;
  - L == 1, and a one-slot window: V's row L - 1 bit for bit, whatever the cap;
  - NaN in the dead slots, the gap slots and behind the page-table entries of the gap pages (and null entries there): the bits
    the clean pages give;
  - a second launch: the same bits; the arrival counters back at zero;
  - one workspace: a plain scan, a capped scan of another shape in the same buffer, the plain scan again;
  - the lean composition, with and without a rotary table: pages, q_output and attention_result bit for bit those of fill ->
    latest -> the capped scan done by hand;
  - every launch counted as "scan_heads_softcap" and no other scan family moved by the capped calls."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import softcap_model as sc
from gpu_util import host
from helpers import assert_equal
from test_alibi_scan_gpu import CASES, FORMS, _counters_are_zero, _newest_v_rows, _pages, _poisoned, length_vectors
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

assert FORMS == sc.FORMS
OTHER_SCAN_FAMILIES = ("scan_heads_window", "scan_heads_alibi", "scan_chunked", "scan_prompt", "scan_prompt_softcap",
                       "scan_equal_shares", "scan_rows_ordered", "scan_rows_grid_order")


def _scaled(x, H, Hkv):
    """the case with q scaled for (H, Hkv): (q on the host, q on the device)"""
    q = sc.scale_q(x.q, x.kt, x.L, H, Hkv)
    return q, _t(q, x.dq.device)


def _capped(ops, x, dq, table, H, Hkv, W, K, cap):
    out = torch.full((x.B, x.D), SENTINEL, device=dq.device)
    ops.decode_scan_paged_softcap(dq, table, x.dL, out, H, Hkv, W, K, cap, ELEM[x.elem], x.S)
    return host(out).copy()


def _plain(ops, x, dq, table, H, Hkv, W, K):
    out = torch.full((x.B, x.D), SENTINEL, device=dq.device)
    ops.decode_scan_paged_gqa(dq, table, x.dL, out, H, Hkv, W, K, ELEM[x.elem], x.S)
    return host(out).copy()


@pytest.mark.parametrize("seed,B,S,D,H,elem,Hkv,chunks", CASES)
def test_softcap_scan(mli, dev, seed, B, S, D, H, elem, Hkv, chunks):
    from min_llm_inference_amd import ops
    failures = []
    launches = 0
    try:
        for part in range(len(length_vectors(seed, B, S))):
            x = _pages(seed, B, S, D, elem, part)
            q, dq = _scaled(x, H, Hkv)
            assert abs(sc.largest_score(q, x.kt, x.L, H, Hkv) - sc.CAPS[0] / 2) < 1e-3
            for W, K in FORMS:
                assert W == 0 or K + W < S
                pool, table_nan, table_null = _poisoned(x, W, K)
                plain = _plain(ops, x, dq, table_nan, H, Hkv, W, K)
                assert mli.mli_launch_counts_reset() == 0
                form_launches = 0
                ones = x.L == 1
                for cap in sc.CAPS:
                    model = sc.SoftcapModel(q, x.kt, x.v, x.L, H, Hkv, cap, W, K)
                    o32 = sc.eval_fp32(q, x.kt, x.v, x.L, H, Hkv, cap, W, K)
                    for ct in chunks:
                        assert mli.mli_tune(b"chunk_tokens", ct) == 0
                        what = f"B{B} S{S} D{D} H{H} Hkv{Hkv} W{W} K{K} {elem} part {part} chunk_tokens {ct} cap {cap:g}"
                        got = _capped(ops, x, dq, table_nan, H, Hkv, W, K, cap)
                        form_launches += 1
                        assert (got[x.L == 0] == 0).all(), f"{what}: rows of length 0"
                        worst, tol = sc.compare(got, o32, model, what=what)
                        if not worst <= tol:
                            failures.append(f"{what}: {worst:.3e} > tol {tol:.3e}")
                        assert_equal(got[ones], _newest_v_rows(x, H, Hkv)[ones], what=f"{what}: L == 1 is V's row 0")
                        if cap != sc.CAPS[1]:
                            continue
                        assert_equal(_capped(ops, x, dq, table_nan, H, Hkv, W, K, cap), got, what=f"{what}: second launch")
                        _counters_are_zero(ops, x, H)
                        assert_equal(_capped(ops, x, dq, x.table, H, Hkv, W, K, cap), got,
                                     what=f"{what}: clean pages against NaN in the dead slots, the gap slots and the gap pages")
                        form_launches += 2
                        if W:
                            assert_equal(_capped(ops, x, dq, table_null, H, Hkv, W, K, cap), got, what=f"{what}: null entries in the gap")
                            form_launches += 1
                        if (x.L > 17).any():
                            assert np.abs(plain - got).max() > 1e-3, f"{what}: the cap changes nothing"
                assert ops.launch_count("scan_heads_softcap") == form_launches
                for family in OTHER_SCAN_FAMILIES:
                    assert ops.launch_count(family) == 0, family
                launches += form_launches
                del pool
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
    assert launches > 0
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("seed,B,S,D,H,elem,Hkv", [(711, 5, 64, 128, 4, "f32", 2), (712, 6, 1024, 256, 8, "bf16", 8),
                                                   (714, 4, 256, 1024, 16, "bf16", 4), (713, 4, 256, 512, 8, "f32", 1)])
def test_a_one_slot_window_gives_the_newest_v_row_bit_for_bit(mli, dev, seed, B, S, D, H, elem, Hkv):
    from min_llm_inference_amd import ops
    for part in range(len(length_vectors(seed, B, S))):
        x = _pages(seed, B, S, D, elem, part)
        _, dq = _scaled(x, H, Hkv)
        pool, table_nan, _ = _poisoned(x, 1, 0)
        for cap in sc.CAPS:
            got = _capped(ops, x, dq, table_nan, H, Hkv, 1, 0, cap)
            assert_equal(got, _newest_v_rows(x, H, Hkv), what=f"B{B} S{S} D{D} H{H} Hkv{Hkv} {elem} W 1 cap {cap:g}")
        del pool


def test_a_plain_call_of_another_shape_shares_the_buffer(mli, dev):
    """One workspace serves both kinds of call: a plain scan, a capped scan of a different shape in the same buffer, the plain
    scan again -- same bits as before, and the capped result within tolerance both times."""
    from min_llm_inference_amd import ops
    y = _pages(712, 6, 1024, 256, "f32", 0)
    H, Hkv, cap = 8, 2, sc.CAPS[1]
    big, _ = ops.workspace_for(y.B, y.S, y.D, dev, H)          # grown once, for the larger need
    x = _pages(711, 5, 64, 128, "f32", 0)
    q, dq = _scaled(y, H, Hkv)
    model, o32 = sc.SoftcapModel(q, y.kt, y.v, y.L, H, Hkv, cap), sc.eval_fp32(q, y.kt, y.v, y.L, H, Hkv, cap)

    def plain():
        out = torch.full((x.B, x.D), SENTINEL, device=dev)
        ops.decode_scan_paged(x.dq, x.table, x.dL, None, out, 0, phases=7, n_sequence=x.S)
        assert ops.workspace_for(x.B, x.S, x.D, dev)[0].data_ptr() == big.data_ptr(), "the calls share one buffer"
        return host(out).copy().view(np.uint32)

    before = plain()
    for what in ("between two plain scans", "after a plain scan"):
        got = _capped(ops, y, dq, y.table, H, Hkv, 0, 0, cap)
        assert ops.workspace_for(y.B, y.S, y.D, dev, H)[0].data_ptr() == big.data_ptr()
        worst, tol = sc.compare(got, o32, model, what=f"capped scan {what}")
        assert worst <= tol
        assert_equal(plain(), before, what=f"plain scan after the capped scan ({what})")


@pytest.mark.parametrize("elem,W,K,rope", [("f32", None, None, False), ("bf16", 40, 4, False), ("f32", 40, 4, True),
                                           ("bf16", None, None, True)])
def test_lean_softcap_composition(oracle, mli, dev, elem, W, K, rope):
    """mli_paged_attention_lean_softcap with new rows, with and without a rotary table: pages and q_output bit-identical to the
    uncapped composition's on the same inputs (fill and projection never see the cap), and attention_result bit-identical to
    mli_decode_scan_paged_softcap run by hand on the pages and the q_output that composition left; the model judges it too."""
    import f64_model as fm
    import rope_model as rp
    from accuracy_cases import dead_slot_offsets, edge_lengths
    from helpers import paged_case
    from min_llm_inference_amd import ops
    seed, B, S, D, H, Hkv, cap = 721, 20, 256, 256, 4, 2, sc.CAPS[2]
    L = edge_lengths(seed, B, S, (64, 44))
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    new = [int(np.nonzero(L == n)[0][0]) for n in (2, 17, 45, 65)]
    c["n_new"] = len(new)
    c["new_batch_idx"][:len(new)] = new
    pool32 = c["pool"].copy()
    oracle.clone_to_pages(pool32, c["table"], c["inp_embedding"], c["kt_cache"], c["v_cache"], L)
    off, _, _ = dead_slot_offsets(c["table"], L, S, D)
    wdt = torch.float32 if elem == "f32" else torch.bfloat16
    table = _t(rp.standard_table(S, D // H), dev) if rope else None

    def run(softcap):
        pool, _ = _poisoned_pool(pool32, off, elem, dev)
        d = SimpleNamespace(pool=pool, q=_t(c["q_output"], dev), out=torch.full((B, D), SENTINEL, device=dev))
        d.table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
        w = [_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv")]
        ops.paged_attention_lean(d.table, _t(L, dev), w[0], w[1], w[2], _t(c["new_batch_idx"], dev), d.q, d.out, c["n_new"], S,
                                 elem=ELEM[elem], n_heads=H, window=W, sinks=K, n_kv_heads=Hkv, rope=table, softcap=softcap)
        torch.cuda.synchronize()
        return d

    plain = run(None)
    assert mli.mli_launch_counts_reset() == 0
    capped = run(cap)
    assert ops.launch_count("scan_heads_softcap") == 1 and ops.launch_count("scan_heads_window") == 0
    if rope:
        assert ops.launch_count("gemm_f32_rope" if elem == "f32" else "gemm_bf16_rope") == 2, "fill_rope, then latest_rope"
    bits = torch.int32 if elem == "f32" else torch.int16
    what = f"lean capped composition {elem} W{W} K{K} rope {rope}"
    assert torch.equal(plain.pool.view(bits), capped.pool.view(bits)), f"{what}: pages do not depend on the cap"
    assert_equal(host(capped.q), host(plain.q), what=f"{what}: q_output does not depend on the cap")
    by_hand = torch.full((B, D), SENTINEL, device=dev)
    ops.decode_scan_paged_softcap(plain.q, plain.table, _t(L, dev), by_hand, H, Hkv, W, K, cap, ELEM[elem], S)
    assert_equal(host(capped.out), host(by_hand), what=f"{what}: fill -> latest -> the capped scan by hand")
    values = torch.nan_to_num(capped.pool.float()).cpu().numpy()
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q = host(capped.q)
    model = sc.SoftcapModel(q, ktm, v_rows, L, H, Hkv, cap, W or 0, K or 0)
    worst, tol = sc.compare(host(capped.out), sc.eval_fp32(q, ktm, v_rows, L, H, Hkv, cap, W or 0, K or 0), model, what=what)
    assert worst <= tol
    assert np.abs(host(capped.out) - host(plain.out)).max() > 1e-4, f"{what}: the cap changes nothing"
