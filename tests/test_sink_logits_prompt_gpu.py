"""The causal multi-query prompt scan with learned attention-sink logits (mli_prompt_scan_paged_sink_logits) and the scoring on top
of it (mli_paged_prompt_logprobs_sink_logits), held to the float64 model with the sink on virtual rows
(tests/sink_logits_model.prompt_model: query t of a segment = the decode model on a row of length t + 1) under the tolerance
derived from its float32 evaluation.

  B, S, D, H / Hkv    pages       kernel variant
  8, 128, 256, 4/2    f32, bf16   one lane load, 8 / 4 queries per workgroup; the query head's logit inside a K/V group
  8, 128, 512, 8/8    f32         two lane loads, 4 queries per workgroup

plain and W 40 with 4 sink tokens, LEARNED and MIXED logits.  The segments' edges are placed by mli_prompt_scan_tq (the variant
keeps it): segments from position 0 and from mid-row, counts tq - 1, tq + 1, tq + 3, 2 tq + 1 (no multiple of tq but one), a
query at n_sequence - 1, rows in permuted order.  NaN above every row's last scored position.  Also: the decode scan with the
same logits on the virtual rows agrees within twice the bound; all -inf gives the plain prompt scan's bits, the -inf and -1e30
heads its bits in their columns, the +1e30 head exact zeros; a second launch gives the same bits; "scan_prompt_sink_logits"
counts the launch and "scan_prompt" does not.  The scoring: token log-probabilities against the float64 scoring
(logprobs_model) of the scan's own result, at the fp32 GEMM's accumulation bound plus the scoring tolerance."""
import numpy as np
import pytest
import torch

import f64_model as fm
import heads_model as hm
import logprobs_model as lm
import prompt_model as pm
import sink_logits_model as sl
from accuracy_cases import fill_pages
from gpu_util import host
from helpers import assert_equal
from test_softcap_prompt_gpu import _case, _distance
from test_window_scan_gpu import ELEM, ESIZE, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

FORMS = ((0, 0), (40, 4))
# (seed, B, S, D, H, Hkv, page type)
CASES = [(841, 8, 128, 256, 4, 2, "f32"), (841, 8, 128, 256, 4, 2, "bf16"), (842, 8, 128, 512, 8, 8, "f32")]
RATIOS = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    RATIOS.clear()
    yield
    if RATIOS:
        print(f"SINK_LOGITS prompt: worst got/tol over {len(RATIOS)} comparisons {max(RATIOS):.3f}")


@pytest.mark.parametrize("seed,B,S,D,H,Hkv,elem", CASES)
def test_prompt_scan_with_sink_logits(oracle, mli, dev, seed, B, S, D, H, Hkv, elem):
    from min_llm_inference_amd import ops
    tq = ops.prompt_scan_tq(D, H, ELEM[elem])
    segs, lengths, c = _case(seed, B, S, D, tq)
    assert any(f == 0 for _, f, _ in segs) and any(f > 0 for _, f, _ in segs) and any(n % tq for _, _, n in segs)
    rows, pos = pm.queries(segs)
    n = len(rows)
    pool32, off = fill_pages(oracle, c, c["q_output"], c["kt_cache"], c["v_cache"])
    pool, values = _poisoned_pool(pool32, off, elem, dev)                 # NaN above every row's last scored position
    ktm = fm.gather_pages(values, c["table"], lengths, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], lengths, S, D, 2)
    nan_page = _nan_page(D, elem, dev)
    table = np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], nan_page.data_ptr()).astype(np.int64)
    qv = pm.query_vectors(c["q_output"], rows, pos)
    q_dev, t_dev = _t(qv, dev), _t(table, dev)
    vt, vL = _t(table[rows], dev), _t((pos + 1).astype(np.int32), dev)
    failures = []
    for W, K in FORMS:
        plain = torch.full((n, D), SENTINEL, device=dev)
        ops.prompt_scan_paged(q_dev, t_dev, segs, plain, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K)
        plain = host(plain).copy()
        z = sl.learned(qv, ktm[rows], pos + 1, H, Hkv, W, K)
        for name, zs, heads in [("LEARNED", z, {})] + [(f"MIXED {i}", zm, hs) for i, (zm, hs) in enumerate(sl.mixed(z))]:
            what = f"B{B} S{S} D{D} H{H}/{Hkv} {elem} W{W} K{K} TQ{tq} | {name}"
            model = sl.prompt_model(qv, ktm, v_rows, rows, pos, H, Hkv, zs, W, K)
            o32 = sl.prompt_eval_fp32(qv, ktm, v_rows, rows, pos, H, Hkv, zs, W, K)
            z_dev = _t(zs, dev)
            out = torch.full((n, D), SENTINEL, device=dev)
            ops.reset_launch_counts()
            ops.prompt_scan_paged(q_dev, t_dev, segs, out, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K, sink_logits=z_dev)
            counts = {f: ops.launch_count(f) for f in ("scan_prompt_sink_logits", "scan_prompt", "scan_prompt_softcap",
                                                       "scan_heads_sink_logits", "scan_heads_window")}
            assert counts == {"scan_prompt_sink_logits": 1, "scan_prompt": 0, "scan_prompt_softcap": 0, "scan_heads_sink_logits": 0,
                              "scan_heads_window": 0}, counts
            got = host(out).copy()
            assert np.isfinite(got).all() and (got != SENTINEL).all(), what
            worst, tol = sl.compare(got, o32, model, what=what)
            RATIOS.append(worst / tol)
            if not worst <= tol:
                failures.append(f"{what}: {worst:.3e} > tol {tol:.3e}")
            for kind, h in heads.items():
                cols = hm.head_slice(h, H, D)
                if kind == "+1e30":
                    assert (got[:, cols] == 0).all(), f"{what}: the +1e30 head is not zero"
                else:
                    assert_equal(got[:, cols], plain[:, cols], what=f"{what}: the {kind} head against the plain prompt scan")
            # the decode scan with the same logits on the virtual rows: row i = the pages of rows[i] with length pos[i] + 1
            ref = torch.full((n, D), SENTINEL, device=dev)
            ops.decode_scan_paged_sink_logits(q_dev, vt, vL, ref, H, Hkv, W, K, z_dev, ELEM[elem], S)
            d = float(_distance(got, host(ref), model).max())
            print(f"SINK_LOGITS PROMPT {what}: {d:.3e} from the decode scan on the virtual rows, twice the bound {2 * tol:.3e}")
            assert d <= 2 * tol, (what, d, tol)
            if name != "LEARNED":
                continue
            sl.conditioned(model, what)
            assert np.abs(got - plain).max() > 1e-3, f"{what}: the logits change nothing"
            again = torch.full((n, D), SENTINEL, device=dev)
            ops.prompt_scan_paged(q_dev, t_dev, segs, again, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K, sink_logits=z_dev)
            assert_equal(host(again), got, what=f"{what}: second launch")
        none = torch.full((n, D), SENTINEL, device=dev)
        ops.prompt_scan_paged(q_dev, t_dev, segs, none, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K,
                              sink_logits=_t(sl.none(H), dev))
        assert_equal(host(none), plain, what=f"B{B} S{S} D{D} H{H}/{Hkv} {elem} W{W} K{K}: all -inf against the plain prompt scan")
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("seed,B,S,D,H,Hkv,elem,W,K", [(841, 8, 128, 256, 4, 2, "f32", 0, 0), (841, 8, 128, 256, 4, 2, "bf16", 40, 4)])
def test_prompt_logprobs_with_sink_logits(oracle, mli, dev, seed, B, S, D, H, Hkv, elem, W, K):
    """mli_paged_prompt_logprobs_sink_logits = projection -> the scan with the logits -> logits -> scoring of
    inp[row, position + 1]: the token log-probabilities against float64 log-softmax of (the scan's result on the projected q) .
    emb^T.  The logits GEMM accumulates emb_dim products in fp32: |logit error| <= emb_dim 2^-24 sum |a e|, twice that for
    logit - lse, plus the scoring's own tolerance (logprobs_model.tolerance).  All -inf: the plain call's bits."""
    from min_llm_inference_amd import ops
    V = 512
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
    z = _t(np.linspace(-1.0, 2.0, H).astype(np.float32), dev)
    ops.reset_launch_counts()
    got = host(ops.paged_prompt_logprobs(table, _t(inp, dev), wq, _t(emb, dev), segs, B, S, ELEM[elem], sink_logits=z, **kw)[0]).copy()
    assert ops.launch_count("scan_prompt_sink_logits") == 1 and ops.launch_count("scan_prompt") == 0
    plain = host(ops.paged_prompt_logprobs(table, _t(inp, dev), wq, _t(emb, dev), segs, B, S, ELEM[elem], **kw)[0]).copy()
    none = host(ops.paged_prompt_logprobs(table, _t(inp, dev), wq, _t(emb, dev), segs, B, S, ELEM[elem],
                                          sink_logits=_t(sl.none(H), dev), **kw)[0]).copy()
    assert_equal(none, plain, what="all -inf against the plain scoring")
    # by hand: the projection, the scan with the logits (held to the model above), then float64
    q = ops.prompt_project_q(table, segs, wq, B, S, ELEM[elem])
    attn = torch.full((n, D), SENTINEL, device=dev)
    ops.prompt_scan_paged(q, table, segs, attn, B, S, ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K, sink_logits=z)
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
    print(f"SINK_LOGITS PROMPT LOGPROBS D{D} H{H}/{Hkv} {elem} W{W} K{K}: error {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert np.abs(got[known] - plain[known]).max() > 4 * bound, "the logits change no figure"
