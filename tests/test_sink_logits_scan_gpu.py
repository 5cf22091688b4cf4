"""The multi-head paged scan with learned attention-sink logits (mli_decode_scan_paged_sink_logits,
mli_paged_attention_lean_sink_logits) held to fp32 rounding error against the float64 model with the sink
(tests/sink_logits_model.py; tests/test_sink_logits_model_cpu.py proves on these very inputs that the comparison bites), on fp32
and bf16 pages; for bf16 pages the model is evaluated on the rounded pool.  The shapes are sink_logits_model.SCAN_SHAPES -- the
smallest at which each mechanism can go wrong:

  B, S, D          H / Hkv (head_dim)          pages       what it reaches
  40, 64, 64       2/2, 2/1 (32)               f32, bf16   one workgroup per row (direct 1); dead lanes
  24, 256, 512     8/8, 8/2 (64); 2/2 (256)    f32, bf16   several items per row: the last arriver's merge, the sink counted once;
                                                           f32: two lane loads; chunk_tokens 0 and 256
  20, 1024, 256    8/2 (32)                    bf16        16 items per row (chunk_tokens 64); the query head's logit in a group
  700, 128, 64     2/2 (32)                    f32         rows handed out longest first (direct 2)

each under (W, n_sink) in {(0, 0), (40, 0), (40, 4)} with accuracy_cases.edge_lengths (0, 1, 2, 15, 16, 17, chunk +- 1, S - 1) and
NaN in the dead K / V slots.  Judged by
  - the model under the tolerance derived from its float32 evaluation, with LEARNED and MIXED logits, under both nt_loads
    settings, where sink_logits_model.conditioned holds (asserted here);
  - NONE (all -inf): the bits of mli_decode_scan_paged_gqa; the -inf and the -1e30 head of MIXED: that call's bits in the head's
    columns; the +1e30 head: exactly 0.0f on every non-empty row; rows of length 0: zero;
  - a second launch: the same bits, and the arrival counters back at zero;
  - "scan_heads_sink_logits" counts exactly the launches made and every other scan family none;
  - WITHOUT the new model (plain form, fp32 pages, no grouping): the scan on rows of L tokens against
    mli_decode_scan_paged_gqa on the same rows lengthened by one crafted token of zero V that scores z_h;
  - the lean composition, with and without a rotary table: bit-identical to fill + latest + the scan called separately."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import f64_model as fm
import gqa_model as gm
import heads_model as hm
import sink_logits_model as sl
from gpu_util import host
from helpers import assert_equal
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

OTHER_SCAN_FAMILIES = ("scan_heads_window", "scan_heads_alibi", "scan_heads_softcap", "scan_chunked", "scan_equal_shares",
                       "scan_rows_ordered", "scan_rows_grid_order", "scan_prompt", "scan_prompt_softcap", "scan_prompt_sink_logits")
RATIOS = []      # got / tol of every comparison of this module, reported at its end


@pytest.fixture(scope="module", autouse=True)
def _report():
    RATIOS.clear()
    yield
    if RATIOS:
        print(f"SINK_LOGITS scan: worst got/tol over {len(RATIOS)} comparisons {max(RATIOS):.3f}")


@functools.lru_cache(maxsize=2)
def _pages(seed, B, S, D, elem):
    """The case's pages in `elem` with NaN in the dead slots, and the values they hold: once per (shape, page type)"""
    c, pool32, dead, L = sl.scan_case(seed, B, S, D)
    dev = torch.device("cuda:0")
    pool, values = _poisoned_pool(pool32, dead, elem, dev)
    q, kt, v, _ = sl.scan_operands(seed, B, S, D, elem, values=np.nan_to_num(values))
    return SimpleNamespace(c=c, L=L, B=B, S=S, D=D, elem=elem, pool=pool, q=q, kt=kt, v=v, dq=_t(q, dev), dL=_t(L, dev),
                           table=_t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev))


def _sink(ops, x, H, Hkv, W, K, z, dq=None, table=None, dL=None, S=None):
    out = torch.full((x.B, x.D), SENTINEL, device=x.dq.device)
    ops.decode_scan_paged_sink_logits(x.dq if dq is None else dq, x.table if table is None else table, x.dL if dL is None else dL,
                                      out, H, Hkv, W, K, _t(np.asarray(z, np.float32), x.dq.device), ELEM[x.elem], S or x.S)
    return host(out).copy()


def _gqa(ops, x, H, Hkv, W, K, table=None, dL=None):
    out = torch.full((x.B, x.D), SENTINEL, device=x.dq.device)
    ops.decode_scan_paged_gqa(x.dq, x.table if table is None else table, x.dL if dL is None else dL, out, H, Hkv, W, K,
                              ELEM[x.elem], x.S)
    return host(out).copy()


def _counters_are_zero(ops, x, H):
    ws, need = ops.workspace_for(x.B, x.S, x.D, x.dq.device, H)
    n = min(need, 65536)
    assert n > 0 and not host(ws[:n]).any(), "the arrival counters are zero between calls"


@pytest.mark.parametrize("seed,B,S,D,H,Hkv,elem,chunks", sl.SCAN_CASES)
def test_sink_logits_scan(mli, dev, seed, B, S, D, H, Hkv, elem, chunks):
    from min_llm_inference_amd import ops
    x = _pages(seed, B, S, D, elem)
    failures = []
    live = x.L > 0
    try:
        for W, K in sl.FORMS:
            assert W == 0 or K + W < S
            z = sl.learned(x.q, x.kt, x.L, H, Hkv, W, K)
            sets = [("LEARNED", z, {})] + [(f"MIXED {i}", zm, heads) for i, (zm, heads) in enumerate(sl.mixed(z))]
            models = {name: sl.SinkLogitsModel(x.q, x.kt, x.v, x.L, H, Hkv, zs, W, K) for name, zs, _ in sets}
            o32 = {name: sl.eval_fp32(x.q, x.kt, x.v, x.L, H, Hkv, zs, W, K) for name, zs, _ in sets}
            sl.conditioned(models["LEARNED"], f"B{B} S{S} D{D} H{H}/{Hkv} W{W} K{K} {elem}")
            for ct in chunks:
                assert mli.mli_tune(b"chunk_tokens", ct) == 0
                plain = _gqa(ops, x, H, Hkv, W, K)
                assert mli.mli_launch_counts_reset() == 0
                launches = 0
                for nt in (0, 1):
                    assert mli.mli_tune(b"nt_loads", nt) == 0
                    for name, zs, heads in sets:
                        what = f"B{B} S{S} D{D} H{H}/{Hkv} W{W} K{K} {elem} chunk_tokens {ct} nt_loads {nt} | {name}"
                        got = _sink(ops, x, H, Hkv, W, K, zs)
                        launches += 1
                        assert (got[~live] == 0).all(), f"{what}: rows of length 0"
                        worst, tol = sl.compare(got, o32[name], models[name], what=what)
                        RATIOS.append(worst / tol)
                        if not worst <= tol:
                            failures.append(f"{what}: {worst:.3e} > tol {tol:.3e}")
                        for kind, h in heads.items():
                            cols = hm.head_slice(h, H, D)
                            if kind == "+1e30":
                                assert np.isfinite(got).all() and (got[live][:, cols] == 0).all(), f"{what}: the +1e30 head is not zero"
                            else:
                                assert_equal(got[:, cols], plain[:, cols], what=f"{what}: the {kind} head against the _gqa call")
                        if name == "LEARNED":
                            assert np.abs(got - plain)[live].max() > 1e-3, f"{what}: the logits change nothing"
                    none = _sink(ops, x, H, Hkv, W, K, sl.none(H))
                    assert_equal(none, plain, what=f"B{B} S{S} D{D} H{H}/{Hkv} W{W} K{K} {elem} chunk_tokens {ct} nt_loads {nt}: "
                                 "all -inf against the _gqa call")
                    launches += 1
                mli.mli_tune(b"nt_loads", 2)
                first = _sink(ops, x, H, Hkv, W, K, z)
                assert_equal(_sink(ops, x, H, Hkv, W, K, z), first, what=f"W{W} K{K} chunk_tokens {ct}: second launch")
                launches += 2
                _counters_are_zero(ops, x, H)
                assert ops.launch_count("scan_heads_sink_logits") == launches
                for family in OTHER_SCAN_FAMILIES:
                    assert ops.launch_count(family) == 0, family
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
        mli.mli_tune(b"nt_loads", 2)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("seed,B,S,D,H,chunks", [(811, 40, 64, 64, 2, (0,)), (812, 24, 256, 512, 8, (0, 64)), (814, 700, 128, 64, 2, (0,))])
def test_the_sink_is_one_more_token_of_zero_v(mli, dev, seed, B, S, D, H, chunks):
    """Independent of sink_logits_model's model: rows of L tokens under the sink-logit scan against mli_decode_scan_paged_gqa on
    the same rows lengthened by sink_logits_model.crafted_token (zero V, K_h = z_h sqrt(hd) q_h / |q_h|^2), plain form, fp32
    pages, no grouping.  Bound: twice the tolerance of the comparison against the model (each kernel is within one of its own
    model) plus the float64 difference of the two models on these pages (the crafted K row is rounded to float32)."""
    from helpers import pool_index
    from min_llm_inference_amd import ops
    x = _pages(seed, B, S, D, "f32")
    z = sl.learned(x.q, x.kt, x.L, H, H)
    rows = np.nonzero((x.L > 0) & (x.L % 16 != 0))[0]          # (room for one more token in the row's last page)
    k_row, v_row = sl.crafted_token(x.q, H, H, z)
    pool = x.pool.clone()
    table = _t(np.where(x.c["table"] >= 0, pool.data_ptr() + 4 * x.c["table"], 0).astype(np.int64), dev)
    longer = x.L.copy()
    kt2 = np.zeros((B, D, x.kt.shape[2] + 16), np.float32)
    v2 = np.zeros((B, x.v.shape[1] + 16, D), np.float32)
    kt2[:, :, :x.kt.shape[2]], v2[:, :x.v.shape[1]] = x.kt, x.v
    for b in rows:
        at = int(pool_index(x.c["table"], b, int(x.L[b]), 0, D))
        assert x.c["table"][b, int(x.L[b]) // 16] >= 0, "the row has a page for one more token"
        pool[at + D:at + 2 * D] = _t(k_row[b], dev)
        pool[at + 2 * D:at + 3 * D] = 0
        kt2[b, :, x.L[b]], v2[b, x.L[b]] = k_row[b], v_row[b]
        longer[b] += 1
    with_sink = sl.SinkLogitsModel(x.q, x.kt, x.v, x.L, H, H, z)
    lengthened = gm.model_gqa(x.q.astype(np.float64), kt2.astype(np.float64), v2.astype(np.float64), longer, H, H)
    tol = sl.tolerance(with_sink, sl.eval_fp32(x.q, x.kt, x.v, x.L, H, H, z))
    between = float(hm.heads_error(lengthened.o, with_sink)[rows].max())
    try:
        for ct in chunks:
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            got = _sink(ops, x, H, H, 0, 0, z)
            out = torch.full((B, D), SENTINEL, device=dev)
            ops.decode_scan_paged_gqa(x.dq, table, _t(longer, dev), out, H, H, 0, 0, ELEM["f32"], S)
            err = float(hm.heads_error(host(out), with_sink)[rows].max())
            mine = float(hm.heads_error(got, with_sink)[rows].max())
            apart = float((np.abs(got - host(out))[rows].reshape(len(rows), H, -1).max(axis=2) / with_sink.o_scale[rows]).max())
            print(f"SINK_LOGITS crafted token B{B} S{S} D{D} H{H} chunk_tokens {ct}: scans apart {apart:.3e}, bound "
                  f"{2 * tol + between:.3e} (tol {tol:.3e}, models apart {between:.3e}); sink scan {mine:.3e}, lengthened {err:.3e}")
            assert apart <= 2 * tol + between
    finally:
        mli.mli_tune(b"chunk_tokens", 0)


@pytest.mark.parametrize("elem,W,K,rope", [("f32", None, None, False), ("bf16", 40, 4, False), ("f32", 40, 4, True),
                                           ("bf16", None, None, True)])
def test_lean_sink_logits_composition(oracle, mli, dev, elem, W, K, rope):
    """mli_paged_attention_lean_sink_logits with new rows, with and without a rotary table: pages and q_output bit-identical to
    the composition's without the logits on the same inputs (fill and projection never see them), and attention_result
    bit-identical to mli_decode_scan_paged_sink_logits run by hand on the pages and the q_output that composition left; the
    model judges it too."""
    import rope_model as rp
    from accuracy_cases import dead_slot_offsets, edge_lengths
    from helpers import paged_case
    from min_llm_inference_amd import ops
    seed, B, S, D, H, Hkv = 821, 20, 256, 256, 4, 2
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

    def run(z):
        pool, _ = _poisoned_pool(pool32, off, elem, dev)
        d = SimpleNamespace(pool=pool, q=_t(c["q_output"], dev), out=torch.full((B, D), SENTINEL, device=dev))
        d.table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
        w = [_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv")]
        ops.paged_attention_lean(d.table, _t(L, dev), w[0], w[1], w[2], _t(c["new_batch_idx"], dev), d.q, d.out, c["n_new"], S,
                                 elem=ELEM[elem], n_heads=H, window=W, sinks=K, n_kv_heads=Hkv, rope=table,
                                 sink_logits=None if z is None else _t(z, dev))
        torch.cuda.synchronize()
        return d

    plain = run(None)
    values = torch.nan_to_num(plain.pool.float()).cpu().numpy()
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q = host(plain.q)
    z = sl.learned(q, ktm, L, H, Hkv, W or 0, K or 0)
    assert mli.mli_launch_counts_reset() == 0
    sunk = run(z)
    assert ops.launch_count("scan_heads_sink_logits") == 1 and ops.launch_count("scan_heads_window") == 0
    if rope:
        assert ops.launch_count("gemm_f32_rope" if elem == "f32" else "gemm_bf16_rope") == 2, "fill_rope, then latest_rope"
    bits = torch.int32 if elem == "f32" else torch.int16
    what = f"lean sink-logit composition {elem} W{W} K{K} rope {rope}"
    assert torch.equal(plain.pool.view(bits), sunk.pool.view(bits)), f"{what}: pages do not depend on the logits"
    assert_equal(host(sunk.q), q, what=f"{what}: q_output does not depend on the logits")
    by_hand = torch.full((B, D), SENTINEL, device=dev)
    ops.decode_scan_paged_sink_logits(plain.q, plain.table, _t(L, dev), by_hand, H, Hkv, W, K, _t(z, dev), ELEM[elem], S)
    assert_equal(host(sunk.out), host(by_hand), what=f"{what}: fill -> latest -> the scan with the logits by hand")
    model = sl.SinkLogitsModel(q, ktm, v_rows, L, H, Hkv, z, W or 0, K or 0)
    sl.conditioned(model, what)
    worst, tol = sl.compare(host(sunk.out), sl.eval_fp32(q, ktm, v_rows, L, H, Hkv, z, W or 0, K or 0), model, what=what)
    RATIOS.append(worst / tol)
    assert worst <= tol
    assert np.abs(host(sunk.out) - host(plain.out)).max() > 1e-3, "the logits change nothing"
