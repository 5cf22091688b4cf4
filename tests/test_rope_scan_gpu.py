"""mli_paged_attention_lean_rope (fill_rope -> latest_rope -> the existing scan router) against the float64 attention model on the
rotated state the call left in memory, at the per-(row, head) tolerance of the heads tests (heads_model.heads_error under
f64_model.tolerance of a float32 numpy evaluation's own error): B 12, S 256, D 128, 4 heads on 4 and on 2 K/V heads -- plain,
W 40, W 40 with 4 sinks, then with ALiBi slopes -- on fp32 and bf16 pages, and one head on fp8 pages.  The state itself is held
to the rotated model by tests/test_rope_gemm_gpu.py; here K of the new rows and q are compared with the un-rotated
composition's (V, x and slot 0 bit-identical, the rest not), and the result with the identity table is that composition's."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import alibi_model as am
import f64_model as fm
import rope_model as rp
from gpu_util import host
from helpers import assert_equal
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

B, S, D = 12, 256, 128
FORMS = [(None, None, False), (40, None, False), (40, 4, False), (40, 4, True), (None, None, True)]
CASES = [("f32", 4, 4), ("f32", 4, 2), ("bf16", 4, 4), ("bf16", 4, 2), ("fp8", 1, 1)]


def _values(pool, elem):
    if elem == "fp8":
        from helpers import fp8_decode
        return fp8_decode(host(pool)).reshape(-1)
    return torch.nan_to_num(pool.float()).cpu().numpy()


NAMES = {(None, None, False): "plain", (40, None, False): "W40", (40, 4, False): "W40-K4", (40, 4, True): "W40-K4-alibi",
         (None, None, True): "alibi"}
# (the single-head scans have no bias: one head runs the forms without slopes)
PARAMS = [pytest.param(e, h, kv, *f, id=f"{e}-H{h}-Hkv{kv}-{NAMES[f]}") for e, h, kv in CASES for f in FORMS if h > 1 or not f[2]]


@pytest.mark.parametrize("elem,H,Hkv,W,K,biased", PARAMS)
def test_lean_rope_composition(oracle, mli, dev, elem, H, Hkv, W, K, biased):
    from accuracy_cases import dead_slot_offsets
    from helpers import paged_case
    from min_llm_inference_amd import ops
    seed = 731
    rng = np.random.default_rng(seed)
    L = rng.integers(S // 2, S, size=B).astype(np.int32)
    L[:8] = [0, 1, 16, 17, 2, 45, 65, S - 1]
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    new = [int(np.nonzero(L == n)[0][0]) for n in (2, 17, 45, 65)]
    c["n_new"] = len(new)
    c["new_batch_idx"][:len(new)] = new
    pool32 = c["pool"].copy()
    oracle.clone_to_pages(pool32, c["table"], c["inp_embedding"], c["kt_cache"], c["v_cache"], L)
    off, _, _ = dead_slot_offsets(c["table"], L, S, D)
    wdt = torch.float32 if elem == "f32" else torch.bfloat16
    slopes = am.standard_slopes(H) if biased else None
    std, ident = rp.standard_table(S, D // H), rp.identity_table(S, D // H)

    def run(table):
        pool, _ = _poisoned_pool(pool32, off, elem, dev)
        d = SimpleNamespace(pool=pool, q=_t(c["q_output"], dev), out=torch.full((B, D), SENTINEL, device=dev))
        ptrs = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64), dev)
        w = [_t(c[k], dev).to(wdt) for k in ("wk", "wq", "wv")]
        kw = dict(elem=ELEM[elem], window=W, sinks=K)
        if H > 1:
            kw.update(n_heads=H, n_kv_heads=Hkv, alibi_slopes=_t(slopes, dev) if biased else None)
        if table is not None:
            kw.update(n_heads=H, rope=_t(table, dev))
        ops.paged_attention_lean(ptrs, _t(L, dev), w[0], w[1], w[2], _t(c["new_batch_idx"], dev), d.q, d.out, c["n_new"], S, **kw)
        torch.cuda.synchronize()
        return d

    assert mli.mli_launch_counts_reset() == 0
    rot = run(std)
    family = "gemm_f32_rope" if elem == "f32" else "gemm_bf16_rope"
    assert ops.launch_count(family) == 2 and ops.launch_count("gemm_f32_panel") == 0, "fill_rope, then latest_rope"
    what = f"lean rope {elem} H{H} Hkv{Hkv} W{W} K{K} {'alibi' if biased else ''}"
    # the attention over the state the call left
    values = _values(rot.pool, elem)
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q = host(rot.q)
    m = slopes if biased else np.zeros(H, np.float32)
    model = am.AlibiModel(q, ktm, v_rows, L, H, Hkv, m, W or 0, K or 0)
    worst, tol = am.compare(host(rot.out), am.eval_fp32(q, ktm, v_rows, L, H, Hkv, m, W or 0, K or 0), model, what=what)
    assert worst <= tol, f"{what}: {worst:.3e} > tol {tol:.3e}"
    assert (host(rot.out)[L == 0] == 0).all()
    # the identity table is the un-rotated composition, bit for bit: pool, q and the attention
    plain, same = run(None), run(ident)
    bits = {"f32": torch.int32, "bf16": torch.int16, "fp8": torch.uint8}[elem]
    assert torch.equal(plain.pool.view(bits), same.pool.view(bits)), f"{what}: identity table: pages"
    assert_equal(host(same.q), host(plain.q), what=f"{what}: identity table: q_output")
    assert_equal(host(same.out), host(plain.out), what=f"{what}: identity table: attention_result")
    # the standard table: rows at slot 0 and empty rows keep q; the others do not; the attention moves
    qs = (host(rot.q).view(np.uint32) == host(plain.q).view(np.uint32)).all(axis=1)
    assert qs[L <= 1].all() and not qs[L > 1].any(), f"{what}: q rows that kept / lost their un-rotated bits"
    assert np.abs(host(rot.out) - host(plain.out)).max() > 1e-3, f"{what}: the rotation changes nothing"
