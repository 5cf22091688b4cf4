"""The causal multi-query prompt scan with logit soft-capping (mli_prompt_scan_paged_softcap) and the scoring on top of it
(mli_paged_prompt_logprobs_softcap), held to the float64 model with the cap on virtual rows (tests/softcap_model.prompt_model:
query t of a segment = the decode model on a row of length t + 1) under the tolerance derived from its float32 evaluation.

  B, S, D, H          pages    kernel variant
  5, 64, 128, 4       f32      one lane load, 8 queries per workgroup
  4, 256, 512, 8      f32      two lane loads, 4
  4, 256, 1024, 16    bf16     two lane loads, 2
  4, 64, 256, 4       bf16     one lane load, 4

each on H and on 2 K/V heads, plain, W 40, W 40 with 4 sinks, at caps 50, 5 and 1, q scaled so that the largest score is half the
largest cap.  The segments' edges are placed by mli_prompt_scan_tq (the capped variants keep it): counts tq - 1, tq, tq + 1 (a
block cut by the end of its segment), 2 tq + 1; a segment continued with seg_first > 0; first positions 0, 15, 16, 17; a query at
n_sequence - 1; rows in permuted order.  NaN above every row's last scored position.  Also: the capped decode scan on the
virtual rows agrees within twice the bound; a second launch gives the same bits; "scan_prompt_softcap" counts the launch and
"scan_prompt" does not.  The scoring: token log-probabilities against float64 logits of the scan's own result, at the fp32 GEMM's
accumulation bound plus the scoring tolerance."""
import functools

import numpy as np
import pytest
import torch

import f64_model as fm
import heads_model as hm
import logprobs_model as lm
import prompt_model as pm
import softcap_model as sc
from accuracy_cases import base_case, fill_pages
from gpu_util import host
from helpers import assert_equal
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

FORMS = ((0, 0), (40, 0), (40, 4))
# (seed, B, S, D, H, page type)
SHAPES = [(741, 5, 64, 128, 4, "f32"), (742, 4, 256, 512, 8, "f32"), (743, 4, 256, 1024, 16, "bf16"), (744, 4, 64, 256, 4, "bf16")]
CASES = [s + (Hkv,) for s in SHAPES for Hkv in (s[4], 2)]


def segments_for(tq, B, S):
    """[(row, first, count)] and the rows' lengths (last scored position + 1; 0 for a row of no segment)"""
    segs = [(2, 16, tq), (0, 0, tq + 3), (3, S - tq - 1, tq + 1), (1, 15, max(tq - 1, 1)), (0, tq + 3, 2 * tq + 1), (1, 17, tq + 1)]
    lengths = np.zeros(B, np.int32)
    for r, f, n in segs:
        lengths[r] = max(lengths[r], f + n)
    assert lengths.max() == S and (lengths <= S).all()
    return segs, lengths


@functools.lru_cache(maxsize=2)
def _case(seed, B, S, D, tq):
    segs, lengths = segments_for(tq, B, S)
    return segs, lengths, base_case(seed, B, S, D, lengths)


def _distance(a, b, model):
    out = np.zeros((a.shape[0], model.H))
    for h in range(model.H):
        sl = hm.head_slice(h, model.H, model.D)
        out[:, h] = np.abs(a[:, sl].astype(np.float64) - b[:, sl]).max(axis=1) / model.o_scale[:, h]
    return out


@pytest.mark.parametrize("seed,B,S,D,H,elem,Hkv", CASES)
def test_capped_prompt_scan(oracle, mli, dev, seed, B, S, D, H, elem, Hkv):
    from min_llm_inference_amd import ops
    tq = ops.prompt_scan_tq(D, H, ELEM[elem])
    segs, lengths, c = _case(seed, B, S, D, tq)
    rows, pos = pm.queries(segs)
    n = len(rows)
    pool32, off = fill_pages(oracle, c, c["q_output"], c["kt_cache"], c["v_cache"])
    pool, values = _poisoned_pool(pool32, off, elem, dev)                 # NaN above every row's last scored position
    ktm = fm.gather_pages(values, c["table"], lengths, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], lengths, S, D, 2)
    nan_page = _nan_page(D, elem, dev)
    table = np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], nan_page.data_ptr()).astype(np.int64)
    qv = sc.scale_q(pm.query_vectors(c["q_output"], rows, pos), ktm[rows], pos + 1, H, Hkv)
    assert abs(sc.largest_score(qv, ktm[rows], pos + 1, H, Hkv) - sc.CAPS[0] / 2) < 1e-3
    q_dev, t_dev = _t(qv, dev), _t(table, dev)
    vt, vL = _t(table[rows], dev), _t((pos + 1).astype(np.int32), dev)
    failures = []
    for W, K in FORMS:
        plain = torch.full((n, D), SENTINEL, device=dev)
        ops.prompt_scan_paged(q_dev, t_dev, segs, plain, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K)
        for cap in sc.CAPS:
            what = f"B{B} S{S} D{D} H{H}/{Hkv} {elem} W{W} K{K} TQ{tq} cap {cap:g}"
            model = sc.prompt_model(qv, ktm, v_rows, rows, pos, H, Hkv, cap, W, K)
            o32 = sc.prompt_eval_fp32(qv, ktm, v_rows, rows, pos, H, Hkv, cap, W, K)
            out = torch.full((n, D), SENTINEL, device=dev)
            ops.reset_launch_counts()
            ops.prompt_scan_paged(q_dev, t_dev, segs, out, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K, softcap=cap)
            counts = {f: ops.launch_count(f) for f in ("scan_prompt_softcap", "scan_prompt", "scan_heads_softcap", "scan_heads_window")}
            assert counts == {"scan_prompt_softcap": 1, "scan_prompt": 0, "scan_heads_softcap": 0, "scan_heads_window": 0}, counts
            got = host(out).copy()
            assert np.isfinite(got).all() and (got != SENTINEL).any(axis=1).all(), what
            worst, tol = sc.compare(got, o32, model, what=what)
            if not worst <= tol:
                failures.append(f"{what}: {worst:.3e} > tol {tol:.3e}")
            if cap != sc.CAPS[1]:
                continue
            assert np.abs(got - host(plain)).max() > 1e-3, f"{what}: the cap changes nothing"
            # the capped decode scan on the virtual rows: row i = the pages of rows[i] with length pos[i] + 1
            ref = torch.full((n, D), SENTINEL, device=dev)
            ops.decode_scan_paged_softcap(q_dev, vt, vL, ref, H, Hkv, W, K, cap, ELEM[elem], S)
            d = float(_distance(got, host(ref), model).max())
            print(f"SOFTCAP PROMPT {what}: {d:.3e} from the capped decode scan on the virtual rows, twice the bound {2 * tol:.3e}")
            assert d <= 2 * tol, (what, d, tol)
            again = torch.full((n, D), SENTINEL, device=dev)
            ops.prompt_scan_paged(q_dev, t_dev, segs, again, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K, softcap=cap)
            assert_equal(host(again), got, what=f"{what}: second launch")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("seed,B,S,D,H,elem,Hkv,W,K", [(741, 5, 64, 128, 4, "f32", 2, 0, 0), (744, 4, 64, 256, 4, "bf16", 4, 40, 4)])
def test_capped_prompt_logprobs(oracle, mli, dev, seed, B, S, D, H, elem, Hkv, W, K):
    """mli_paged_prompt_logprobs_softcap = projection -> the capped scan -> logits -> scoring of inp[row, position + 1]: the token
    log-probabilities against float64 log-softmax of (the capped scan's result on the projected q) . emb^T.  The logits GEMM
    accumulates emb_dim products in fp32: |logit error| <= emb_dim 2^-24 sum |a e|, twice that for logit - lse, plus the
    scoring's own tolerance (logprobs_model.tolerance).  Without the cap the figures differ."""
    from min_llm_inference_amd import ops
    V, cap = 512, sc.CAPS[2]
    tq = ops.prompt_scan_tq(D, H, ELEM[elem])
    segs, lengths, c = _case(seed, B, S, D, tq)
    rows, pos = pm.queries(segs)
    n = len(rows)
    pool32, off = fill_pages(oracle, c, c["q_output"], c["kt_cache"], c["v_cache"])
    pool, _ = _poisoned_pool(pool32, off, elem, dev)
    nan_page = _nan_page(D, elem, dev)
    table = _t(np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], nan_page.data_ptr()).astype(np.int64), dev)
    rng = np.random.default_rng(seed)
    emb = (rng.standard_normal((V, D)) * 0.5).astype(np.float32)
    inp = rng.integers(0, V, size=(B, S)).astype(np.int32)
    wq = _t((rng.standard_normal((D, D)) * (2.0 / np.sqrt(D))).astype(np.float32), dev).to(torch.float32 if elem == "f32" else torch.bfloat16)
    kw = dict(n_top=0, n_heads=H, n_kv_heads=Hkv, window=W, sinks=K)
    ops.reset_launch_counts()
    got = host(ops.paged_prompt_logprobs(table, _t(inp, dev), wq, _t(emb, dev), segs, B, S, ELEM[elem], softcap=cap, **kw)[0]).copy()
    assert ops.launch_count("scan_prompt_softcap") == 1 and ops.launch_count("scan_prompt") == 0
    plain = host(ops.paged_prompt_logprobs(table, _t(inp, dev), wq, _t(emb, dev), segs, B, S, ELEM[elem], **kw)[0]).copy()
    # by hand: the projection, the capped scan (held to the model above), then float64
    q = ops.prompt_project_q(table, segs, wq, B, S, ELEM[elem])
    attn = torch.full((n, D), SENTINEL, device=dev)
    ops.prompt_scan_paged(q, table, segs, attn, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K, softcap=cap)
    a64, e64 = host(attn).astype(np.float64), emb.astype(np.float64)
    logits = a64 @ e64.T
    gemm = D * 2.0 ** -24 * (np.abs(a64) @ np.abs(e64).T).max()
    m = logits.max(axis=1, keepdims=True)
    lp64 = logits - m - np.log(np.exp(logits - m).sum(axis=1, keepdims=True))
    given = np.asarray([inp[r, t + 1] if t + 1 < S else -1 for r, t in zip(rows, pos)], np.int64)
    known = given >= 0
    assert (~known).sum() == 1 and (got[~known] == -np.inf).all(), "the query at n_sequence - 1 has no next token"
    err = float(np.abs(got[known] - lp64[np.arange(n)[known], given[known]]).max())
    bound = 2 * gemm + lm.tolerance(logits.astype(np.float32))
    print(f"SOFTCAP PROMPT LOGPROBS D{D} H{H}/{Hkv} {elem} W{W} K{K}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.abs(got[known] - plain[known]).max() > 4 * bound, "the cap changes no figure"
