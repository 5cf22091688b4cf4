"""Every instantiation of the four multi-head decode scan kernel templates (attention_heads.hpp) launched once and judged:

  heads_decode_scan_kernel / heads_alibi_scan_kernel / heads_softcap_scan_kernel / heads_sink_logits_scan_kernel
      <E, NJ, NT, WIN, SINK, GQA>:  E {f32, bf16} x NJ {1, 2} x NT {0, 1} x {plain, window, window + sink tokens} x GQA {0, 1}

4 x 48 = 192 kernels.  The family files (test_gqa_scan_gpu.py, test_alibi_scan_gpu.py, test_softcap_scan_gpu.py,
test_sink_logits_scan_gpu.py) choose their shapes for the mechanisms; at those shapes nt_loads_rule (scan_plan.hpp) never picks
NT = 1 by itself, and only some of them force it.  This file enumerates the template space instead, at the smallest shapes that
reach each instantiation and its merge:

  B 6, S 128, lengths 0, 1, 16, 17, S - 1, S;  (W, K) in (0, 0), (40, 0), (40, 4);  n_kv_heads in {H, 1}
  chunk_tokens 64 (several items per row, the last arriver's merge) and 0 (one workgroup per row);  nt_loads 0 and 1

  pages   NJ   D      H     (NJ = ceil(D / elements per 16-byte lane load / 64), asserted)
  f32     1    64     2
  f32     2    512    2
  bf16    1    64     2
  bf16    2    1024   4

Each launch is judged by its family's own float64 model, generator and tolerance, unchanged: gqa_model (oracle-derived
tolerance per score family), alibi_model with the standard slopes, softcap_model at cap 5 on q scaled by softcap_model.scale_q,
sink_logits_model with LEARNED logits where sink_logits_model.conditioned holds (asserted); for bf16 pages the model is evaluated
on the rounded pool; the dead slots, the gap slots and the gap pages hold NaN.  Also: nt_loads 1 gives the bits of nt_loads 0
(DESIGN 3.8), rows of length 0 are exact zeros, a second launch gives the same bits, the family's launch counter equals the
launches made and no other multi-head family moves, and the tune knobs are restored."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import alibi_model as am
import f64_model as fm
import gqa_model as gm
import sink_logits_model as sl
import softcap_model as sc
from accuracy_cases import base_case, fill_pages
from gpu_util import host
from helpers import assert_equal
from test_alibi_scan_gpu import _poisoned
from test_window_scan_gpu import ELEM, SENTINEL, _nan_page, _poisoned_pool, _t

pytestmark = pytest.mark.gpu

B, S = 6, 128
LENGTHS = (0, 1, 16, 17, S - 1, S)
FORMS = ((0, 0), (40, 0), (40, 4))
CHUNKS = (64, 0)
COUNTER = {"plain": "scan_heads_window", "alibi": "scan_heads_alibi", "softcap": "scan_heads_softcap",
           "sink_logits": "scan_heads_sink_logits"}
WIDTHS = {("f32", 1): (64, 2), ("f32", 2): (512, 2), ("bf16", 1): (64, 2), ("bf16", 2): (1024, 4)}     # (D, H)
EPL = {"f32": 4, "bf16": 8}
CAP = sc.CAPS[1]
assert CAP == 5.0


@functools.lru_cache(maxsize=2)
def _pages(D, elem):
    """The case's pages in `elem` and the values they hold: once per (width, page type), shared by the four families"""
    import oracle
    oracle.lib()
    L = np.asarray(LENGTHS, np.int32)
    c = base_case(900 + D, B, S, D, L)
    pool32, dead = fill_pages(oracle, c, c["q_output"], c["kt_cache"], c["v_cache"])
    dev = torch.device("cuda:0")
    clean, values = _poisoned_pool(pool32, np.zeros(0, np.int64), elem, dev)
    return SimpleNamespace(c=c, L=L, B=B, S=S, D=D, elem=elem, pool32=pool32, dead=dead, clean=clean, q=c["q_output"],
                           kt=fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1),
                           v=fm.gather_pages(values, c["table"], L, S, D, 2), dq=_t(c["q_output"], dev), dL=_t(L, dev),
                           nan_page=_nan_page(D, elem, dev))


def _family(family, oracle, ops, x, H, Hkv, W, K):
    """(launch(table) -> attention_result on the host, judge(got, what) -> [(worst, tol)]) of one family at one form"""
    dev = x.dq.device

    def run(call, dq, *extra):
        def launch(table):
            out = torch.full((x.B, x.D), SENTINEL, device=dev)
            call(dq, table, x.dL, out, H, Hkv, W, K, *extra, ELEM[x.elem], x.S)
            return host(out).copy()
        return launch

    if family == "plain":
        model, want = gm.model_gqa(x.q, x.kt, x.v, x.L, H, Hkv, W, K), gm.oracle_gqa(oracle, x.q, x.kt, x.v, x.L, H, Hkv, W, K)
        return (run(ops.decode_scan_paged_gqa, x.dq),
                lambda got, what: [(w, t) for _, w, t in gm.compare(got, want, model, ("flat",) * H, what=what)])
    if family == "alibi":
        m = am.standard_slopes(H)
        model, o32 = am.AlibiModel(x.q, x.kt, x.v, x.L, H, Hkv, m, W, K), am.eval_fp32(x.q, x.kt, x.v, x.L, H, Hkv, m, W, K)
        return (run(ops.decode_scan_paged_alibi, x.dq, _t(np.asarray(m, np.float32), dev)),
                lambda got, what: [am.compare(got, o32, model, what=what)])
    if family == "softcap":
        q = sc.scale_q(x.q, x.kt, x.L, H, Hkv)
        model, o32 = sc.SoftcapModel(q, x.kt, x.v, x.L, H, Hkv, CAP, W, K), sc.eval_fp32(q, x.kt, x.v, x.L, H, Hkv, CAP, W, K)
        return (run(ops.decode_scan_paged_softcap, _t(q, dev), CAP),
                lambda got, what: [sc.compare(got, o32, model, what=what)])
    assert family == "sink_logits"
    z = sl.learned(x.q, x.kt, x.L, H, Hkv, W, K)
    model, o32 = sl.SinkLogitsModel(x.q, x.kt, x.v, x.L, H, Hkv, z, W, K), sl.eval_fp32(x.q, x.kt, x.v, x.L, H, Hkv, z, W, K)
    sl.conditioned(model, f"D{x.D} H{H}/{Hkv} W{W} K{K} {x.elem}")
    return (run(ops.decode_scan_paged_sink_logits, x.dq, _t(z, dev)),
            lambda got, what: [sl.compare(got, o32, model, what=what)])


@pytest.mark.parametrize("nj", (1, 2))
@pytest.mark.parametrize("elem", ("f32", "bf16"))
@pytest.mark.parametrize("family", tuple(COUNTER))
def test_every_instantiation_is_judged(oracle, mli, dev, family, elem, nj):
    from min_llm_inference_amd import ops
    D, H = WIDTHS[elem, nj]
    assert -(-(D // EPL[elem]) // 64) == nj, "the width gives the wanted NJ"
    x = _pages(D, elem)
    empty = x.L == 0
    assert empty.any() and x.L.max() == S
    failures, ratios, launches = [], [], 0
    assert mli.mli_launch_counts_reset() == 0
    try:
        for Hkv in (H, 1):                                   # GQA off / on
            for W, K in FORMS:                               # plain / WIN / WIN + SINK
                assert W == 0 or K + W < S
                pool, table_nan, _ = _poisoned(x, W, K)
                launch, judge = _family(family, oracle, ops, x, H, Hkv, W, K)
                for ct in CHUNKS:
                    assert mli.mli_tune(b"chunk_tokens", ct) == 0
                    got = {}
                    for nt in (0, 1):                        # NT off / on
                        assert mli.mli_tune(b"nt_loads", nt) == 0
                        what = f"{family} {elem} NJ{nj} D{D} H{H}/{Hkv} W{W} K{K} chunk_tokens {ct} nt_loads {nt}"
                        got[nt] = launch(table_nan)
                        launches += 1
                        assert (got[nt][empty] == 0).all(), f"{what}: rows of length 0"
                        assert np.isfinite(got[nt]).all() and (got[nt] != SENTINEL).all(), what
                        for worst, tol in judge(got[nt], what):
                            ratios.append(worst / tol)
                            if not worst <= tol:
                                failures.append(f"{what}: {worst:.3e} > tol {tol:.3e}")
                        assert_equal(launch(table_nan), got[nt], what=f"{what}: second launch")
                        launches += 1
                    assert_equal(got[1], got[0], what=f"{what}: nt_loads 1 against nt_loads 0")
                del pool
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
        mli.mli_tune(b"nt_loads", 2)
    for name, counter in COUNTER.items():
        assert ops.launch_count(counter) == (launches if name == family else 0), counter
    assert launches == 2 * len(FORMS) * len(CHUNKS) * 2 * 2
    print(f"HEADS_INSTANTIATIONS {family} {elem} NJ{nj}: worst got/tol {max(ratios):.3f} over {len(ratios)} comparisons")
    assert not failures, "\n".join(failures)
