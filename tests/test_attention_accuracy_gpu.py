"""The attention kernels held to fp32 rounding error against the float64 model (tests/f64_model.py), DESIGN 6.

Every other parity test compares with the fp32 oracle at 1e-3 ABSOLUTE -- the reference's threshold, made for its
U(0, 1] data.  On long, well-conditioned rows (p ~ 1 / L, outputs ~ 0.01 .. 0.1) that is 1 - 10 % of the signal: a scan
that drops the last token of a row passes.  Here every entry point that computes scores, probabilities or
attention_result is compared on EVERY row with a per-row, condition-scaled error, and the tolerance of a case is
computed in the test from the fp32 CPU oracle's own error against the same model on the same inputs:
tol = max(8 x E_oracle, 16 x 2^-24) -- never from a kernel.  tests/test_accuracy_model_cpu.py proves that the comparison
fails for nine kinds of subtly wrong attention.

Dead slots (s >= L): NaN in K and V for the paged scans (scan_item_body.hpp: "never multiply unwritten page memory, even
by zero"); for the contiguous kernels, the standalone three-stage kernels and the compositions a K that would score +80
with V = 1e30 (finite: a multiply-by-zero mask is legal there, an included token is gross).

Set MLI_ACCURACY_REPORT=<file> to get the measured errors per (path, page type, family) as JSON (the table of DESIGN 6)."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import f64_model as fm
from accuracy_cases import (FAMILIES, SCAN_SHAPES, STREAM_CASES, apply_family, base_case, edge_lengths, fill_pages,
                            oracle_scan, poison_contiguous)
from accuracy_gpu import (ELEM, REPORT as _report, SENTINEL, Checker, elems_for as _elems_for, lean as _lean,
                          lean_twice as _lean_twice, paged_inputs as _paged_inputs, to_device as _t)
from gpu_util import host
from helpers import assert_equal, paged_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("MLI_ACCURACY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({" | ".join(k): v for k, v in sorted(_report.items())}, f, indent=1)


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, chunks, lengths=None):
    if isinstance(lengths, tuple):
        L = np.asarray(lengths, np.int32)
    else:
        L = edge_lengths(seed, B, S, chunks, short=lengths == "short")
    return base_case(seed, B, S, D, L)


def _two_rows_of_S_tokens(L, S):
    """The length vector with its two long random rows (>= 3/4 S) made full: L == n_sequence, all S / 16 pages present.
    Every paged scan clamps with min(L, S); the reference's own wrapper never goes beyond S - 1."""
    L = L.copy()
    rows = np.nonzero((L >= 3 * S // 4) & (L < S - 2))[0][:2]
    assert len(rows) == 2
    L[rows] = S
    return L


@functools.lru_cache(maxsize=1)
def _base_to_S(seed, B, S, D, chunks):
    return base_case(seed, B, S, D, _two_rows_of_S_tokens(edge_lengths(seed, B, S, chunks), S))


# ---- the single-pass paged scan (chunked grid): materialising and lean, fp32 / bf16 / fp8 pages ---------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed,B,S,D,chunks", SCAN_SHAPES)
def test_paged_scan(oracle, mli, dev, seed, B, S, D, chunks, family):
    from min_llm_inference_amd import ops
    c = _base(seed, B, S, D, chunks)
    for elem in _elems_for(D):
        ck = Checker(family, elem)
        x = _paged_inputs(oracle, dev, c, family, elem)
        _, p_or, o_or = x.oracle
        e_o, e_p = fm.attention_error(o_or, x.model), fm.probability_error(p_or, x.model)
        try:
            assert mli.mli_tune(b"scan_stream", 0) == 0
            if elem != "fp8":        # (the fp8 extension has the lean form only)
                qkt = torch.full((B, S), SENTINEL, device=dev)
                out = torch.full((B, D), SENTINEL, device=dev)
                ops.decode_scan_paged(x.q, x.page_table, x.L, qkt, out, ELEM[elem], phases=3)
                ck.check("paged scan, materialising", "attention", fm.attention_error(host(out), x.model), e_o)
                ck.check("paged scan, materialising", "probabilities", fm.probability_error(host(qkt), x.model), e_p)
            for merge in (1, 0):
                assert mli.mli_tune(b"scan_merge", merge) == 0
                got = _lean_twice(ops, x, elem, f"lean, scan_merge {merge}")
                ck.check("paged scan, lean", "attention", fm.attention_error(got, x.model), e_o)
            mli.mli_tune(b"scan_merge", 1)
            for nt in (0, 1):
                assert mli.mli_tune(b"nt_loads", nt) == 0
                ck.check("paged scan, lean", "attention", fm.attention_error(_lean(ops, x, elem), x.model), e_o)
            mli.mli_tune(b"nt_loads", 2)
            if S <= 128 and B > 512:   # one workgroup per row, rows handed out longest first by default: grid order too
                assert mli.mli_tune(b"scan_row_order", 0) == 0
                ck.check("paged scan, lean", "attention", fm.attention_error(_lean(ops, x, elem), x.model), e_o)
        finally:
            mli.mli_tune(b"scan_stream", 1)
            mli.mli_tune(b"scan_merge", 1)
            mli.mli_tune(b"nt_loads", 2)
            mli.mli_tune(b"scan_row_order", 1)
        ck.done()


@pytest.mark.parametrize("family", FAMILIES)
def test_paged_scan_with_rows_of_S_tokens(oracle, mli, dev, family):
    """mli_decode_scan_paged, materialising and lean (chunked grid), on the S = 1024 shape with two rows of 1024 tokens."""
    from min_llm_inference_amd import ops
    seed, B, S, D, chunks = SCAN_SHAPES[1]
    c = _base_to_S(seed, B, S, D, chunks)
    for elem in _elems_for(D):
        ck = Checker(family, elem)
        x = _paged_inputs(oracle, dev, c, family, elem)
        assert x.lengths.max() == S and (x.lengths == S).sum() == 2 and x.lengths.min() == 0
        e_o, e_p = fm.attention_error(x.oracle[2], x.model), fm.probability_error(x.oracle[1], x.model)
        try:
            assert mli.mli_tune(b"scan_stream", 0) == 0
            if elem != "fp8":
                qkt = torch.full((B, S), SENTINEL, device=dev)
                out = torch.full((B, D), SENTINEL, device=dev)
                ops.decode_scan_paged(x.q, x.page_table, x.L, qkt, out, ELEM[elem], phases=3)
                ck.check("paged scan, materialising, L = S", "attention", fm.attention_error(host(out), x.model), e_o)
                ck.check("paged scan, materialising, L = S", "probabilities", fm.probability_error(host(qkt), x.model), e_p)
            got = _lean_twice(ops, x, elem, "lean, rows of S tokens")
            ck.check("paged scan, lean, L = S", "attention", fm.attention_error(got, x.model), e_o)
        finally:
            mli.mli_tune(b"scan_stream", 1)
        ck.done()


def test_the_comparison_sees_a_scan_that_stops_one_token_early(oracle, mli, dev):
    """The comparison checked against itself on the device: the lean scan given lengths - 1 IS the "last token dropped"
    mutant of tests/test_accuracy_model_cpu.py.  Against the model of the true lengths every non-empty row must be off by
    at least 4x the tolerance -- the 4095-token rows included, where the absolute difference is ~ 2.5e-4 and 1e-3 sees
    nothing."""
    from min_llm_inference_amd import ops
    seed, B, S, D, chunks = SCAN_SHAPES[2]
    x = _paged_inputs(oracle, dev, _base(seed, B, S, D, chunks), "flat", "f32")
    tol = fm.tolerance(fm.attention_error(x.oracle[2], x.model))
    out = torch.full((B, D), SENTINEL, device=dev)
    ops.decode_scan_paged(x.q, x.page_table, _t(np.maximum(x.lengths - 1, 0).astype(np.int32), dev), None, out, 0, phases=7,
                          n_sequence=S)
    err = fm.attention_error(host(out), x.model)
    live = x.lengths >= 1
    assert x.lengths.max() == S - 1 and (err[live] >= 4 * tol).all(), (err[live].min(), tol)
    assert np.abs(host(out)[x.lengths >= S - 2] - x.model.o[x.lengths >= S - 2]).max() < 1e-3, "... which 1e-3 absolute lets pass"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("chunk", [64, 1024])
def test_paged_scan_forced_chunks(oracle, mli, dev, chunk, family):
    """chunk_tokens 64 (64 partials per row) and 1024 at S = 4096, lengths on and around both chunk sizes."""
    from min_llm_inference_amd import ops
    B, S, D = 18, 4096, 128
    c = _base(141, B, S, D, (64, 1024))
    for elem in _elems_for(D):
        ck = Checker(family, elem)
        x = _paged_inputs(oracle, dev, c, family, elem)
        e_o, e_p = fm.attention_error(x.oracle[2], x.model), fm.probability_error(x.oracle[1], x.model)
        try:
            assert mli.mli_tune(b"scan_stream", 0) == 0
            assert mli.mli_tune(b"chunk_tokens", chunk) == 0
            if elem != "fp8":
                qkt = torch.full((B, S), SENTINEL, device=dev)
                out = torch.full((B, D), SENTINEL, device=dev)
                ops.decode_scan_paged(x.q, x.page_table, x.L, qkt, out, ELEM[elem], phases=3)
                ck.check(f"paged scan, chunk_tokens {chunk}", "attention", fm.attention_error(host(out), x.model), e_o)
                ck.check(f"paged scan, chunk_tokens {chunk}", "probabilities", fm.probability_error(host(qkt), x.model), e_p)
            got = _lean_twice(ops, x, elem, f"lean, chunk_tokens {chunk}")
            ck.check(f"paged scan, chunk_tokens {chunk}", "attention", fm.attention_error(got, x.model), e_o)
        finally:
            mli.mli_tune(b"chunk_tokens", 0)
            mli.mli_tune(b"scan_stream", 1)
        ck.done()


# ---- the equal-page-shares scan (attention_stream.hip): the kernel the headline number is quoted on ---------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed,B,S,D,lengths", STREAM_CASES)
def test_equal_page_shares_scan(oracle, mli, dev, seed, B, S, D, lengths, family):
    from min_llm_inference_amd import ops
    c = _base(seed, B, S, D, () if lengths == "short" else (64, 256), tuple(lengths) if isinstance(lengths, list) else lengths)
    for elem in _elems_for(D):
        ck = Checker(family, elem)
        x = _paged_inputs(oracle, dev, c, family, elem)
        e_o = fm.attention_error(x.oracle[2], x.model)
        try:
            assert mli.mli_tune(b"scan_stream", 1) == 0
            assert mli.mli_tune(b"scan_stream_min_tokens", 0) == 0
            assert mli.mli_tune(b"scan_stream_granule", 16) == 0
            for dyn in (12, 0):            # 12: static shares + granules handed out by ticket; 0: static shares only
                assert mli.mli_tune(b"scan_stream_dynamic_pct", dyn) == 0
                got = _lean_twice(ops, x, elem, f"equal shares, dynamic {dyn} %")
                ck.check("equal-page-shares scan", "attention", fm.attention_error(got, x.model), e_o)
        finally:
            mli.mli_tune(b"scan_stream", 1)
            mli.mli_tune(b"scan_stream_min_tokens", 1 << 21)
            mli.mli_tune(b"scan_stream_dynamic_pct", 4)
            mli.mli_tune(b"scan_stream_granule", 64)
        ck.done()


# ---- the standalone three-stage kernels and the contiguous single-launch scan -------------------------------------------
STAGE_SHAPES = [s for s in SCAN_SHAPES if s[0] in (131, 132, 133, 134, 135, 136)]


def _stage_models(oracle, q, kt, v, L):
    """Each stage fed the MODEL's previous stage rounded to fp32, so that a stage's error is its own: (model, fp32 scores in,
    stage model of the softmax, its oracle error, fp32 probabilities in, stage model of p.V, its oracle error)."""
    m = fm.Model(q, kt, v, L)
    S = kt.shape[2]
    dead = np.arange(S)[None, :] >= np.asarray(L)[:, None]
    x32 = m.x.astype(np.float32)
    x32[dead] = 80.0                                 # a dead score that would dominate the row if it were included
    ms = SimpleNamespace(lengths=m.lengths, p=fm.softmax(x32.astype(np.float64), L))
    p_or = x32.copy()
    oracle.softmax_in_place_with_lengths_host(p_or, np.ascontiguousarray(L, np.int32))
    p32 = m.p.astype(np.float32)
    mv = SimpleNamespace(lengths=m.lengths, o=fm.attend(p32, v, L), o_scale=fm.attend_abs(p32, v, L).max(axis=1))
    o_or = np.zeros((len(L), v.shape[2]), np.float32)
    oracle.softmax_v_host(p32, np.ascontiguousarray(v, np.float32), o_or, np.ascontiguousarray(L, np.int32))
    return m, x32, ms, fm.probability_error(p_or, ms), p32, mv, fm.attention_error(o_or, mv)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed,B,S,D,chunks", STAGE_SHAPES)
def test_contiguous_stages_and_scan(oracle, mli, dev, seed, B, S, D, chunks, family):
    """launch_qkt, launch_softmax_in_place_with_lengths, launch_softmax_v and decode_scan_contiguous; one row is full (L = S)."""
    from min_llm_inference_amd import ops
    c = _base(seed, B, S, D, chunks)
    q, kt = apply_family(c, family)
    v = c["v_cache"].copy()
    L = c["lengths"].copy()
    L[-1] = S                                        # the contiguous entry points allow a full row
    poison_contiguous(q, kt, v, L)
    ck = Checker(family)
    m, x32, ms, e_soft, p32, mv, e_pv = _stage_models(oracle, q, kt, v, L)
    x_or, _, o_or = oracle_scan(oracle, q, kt, v, L)
    dq, dkt, dv, dL = _t(q, dev), _t(kt, dev), _t(v, dev), _t(L, dev)
    dead = np.arange(S)[None, :] >= L[:, None]
    qkt = torch.full((B, S), SENTINEL, device=dev)
    ops.launch_qkt(dq, dkt, dL, qkt)
    got = host(qkt)
    ck.check("launch_qkt", "scores", fm.score_error(got, m), fm.score_error(x_or, m))
    assert (got[dead] == SENTINEL).all(), "launch_qkt writes nothing at s >= L"
    probs = _t(x32, dev)
    ops.launch_softmax_in_place_with_lengths(probs, dL)
    ck.check("launch_softmax_in_place_with_lengths", "probabilities", fm.probability_error(host(probs), ms), e_soft)
    out = torch.full((B, D), SENTINEL, device=dev)
    ops.launch_softmax_v(_t(p32, dev), dv, out, dL)
    ck.check("launch_softmax_v", "attention", fm.attention_error(host(out), mv), e_pv)
    e_o = fm.attention_error(o_or, m)
    outs = []
    for _ in range(2):                               # the rows' arrival counters are back at zero
        out.fill_(SENTINEL)
        ops.decode_scan_contiguous(dq, dkt, dv, dL, out)
        outs.append(host(out).copy())
    assert_equal(outs[1], outs[0], what="decode_scan_contiguous: second launch")
    ck.check("decode_scan_contiguous", "attention", fm.attention_error(outs[0], m), e_o)
    ck.done()


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed,B,S,D,chunks", STAGE_SHAPES)
def test_paged_stages(oracle, mli, dev, seed, B, S, D, chunks, family):
    """launch_qkt_paged_attention[_bf16] and launch_softmax_v_paged_attention[_bf16] on fp32 and bf16 pages."""
    from min_llm_inference_amd import ops
    c = _base(seed, B, S, D, chunks)
    for elem in ("f32", "bf16"):
        ck = Checker(family, elem)
        x = _paged_inputs(oracle, dev, c, family, elem, poison="finite")
        ktm = x.k_rows.transpose(0, 2, 1)
        m, _, _, _, p_live, mv, e_pv = _stage_models(oracle, x.q_host, ktm, x.v_rows, x.lengths)
        p32 = np.zeros((B, S), np.float32)               # (the model's arrays end at the longest row)
        p32[:, :p_live.shape[1]] = p_live
        dead = np.arange(S)[None, :] >= x.lengths[:, None]
        qkt = torch.full((B, S), SENTINEL, device=dev)
        out = torch.full((B, D), SENTINEL, device=dev)
        f_qkt, f_pv = ((ops.launch_qkt_paged_attention, ops.launch_softmax_v_paged_attention) if elem == "f32" else
                       (ops.launch_qkt_paged_attention_bf16, ops.launch_softmax_v_paged_attention_bf16))
        f_qkt(x.q, x.page_table, x.L, qkt)
        got = host(qkt)
        ck.check("launch_qkt_paged_attention", "scores", fm.score_error(got, m), fm.score_error(x.oracle[0], m))
        assert (got[dead] == SENTINEL).all(), "the paged q.K^T writes nothing at s >= L"
        f_pv(_t(p32, dev), x.page_table, out, x.L)
        ck.check("launch_softmax_v_paged_attention", "attention", fm.attention_error(host(out), mv), e_pv)
        ck.done()


# ---- the non-temporal instantiations (tests/kernel_coverage.json) ------------------------------------------------------------
# By itself nt_loads_rule (scan_plan.hpp) picks non-temporal K / V loads beyond 768 MiB of K / V only; the cases below force them
# with mli_tune "nt_loads" = 1 at the smallest shapes that reach each kernel, under the judges above.
@pytest.mark.parametrize("seed,B,S,D,chunks", [s for s in SCAN_SHAPES if s[0] in (131, 134, 135)])
def test_stages_and_contiguous_scan_with_non_temporal_loads(oracle, mli, dev, seed, B, S, D, chunks):
    """test_contiguous_stages_and_scan and test_paged_stages under nt_loads 1.  There for
    D 64:   softmax_v_partial_kernel<4, 1, false, true> (contiguous) and <4, 1, true, true> (paged);
    D 512:  softmax_v_partial_kernel<4, 2, false, true>, naive_decode_scan_kernel<2, true>;
    D 2048: softmax_v_partial_bf16_kernel<2, true>."""
    try:
        assert mli.mli_tune(b"nt_loads", 1) == 0
        test_contiguous_stages_and_scan(oracle, mli, dev, seed, B, S, D, chunks, "flat")
        test_paged_stages(oracle, mli, dev, seed, B, S, D, chunks, "flat")
    finally:
        mli.mli_tune(b"nt_loads", 2)


@pytest.mark.parametrize("elem,D", [("f32", 512), ("f32", 1024), ("bf16", 1024), ("bf16", 2048), ("bf16", 4096)])
def test_paged_scan_materialising_with_non_temporal_loads(oracle, mli, dev, elem, D):
    """mli_decode_scan_paged, materialising and lean (chunked grid), under nt_loads 1: B 14, S 128 (two items per row).  There for
    fused_decode_scan_kernel<E, NJ, NT = true, TBR, DS, SCORES, 1> with SCORES = true, which test_paged_scan runs under the default
    policy only -- f32 D 512: <ElemF32, 2, true, 4, false, true, 1>; f32 D 1024 (the waves split the row): <ElemF32, 1, true, 8, true,
    true, 1>; bf16 D 1024: <ElemBF16, 2, true, 4, false, true, 1>; bf16 D 2048: <ElemBF16, 1, true, 8, true, true, 1>; bf16 D 4096:
    <ElemBF16, 2, true, 4, true, true, 1> and the lean <ElemBF16, 2, true, 4, true, false, 1>."""
    from min_llm_inference_amd import ops
    B, S = 14, 128
    x = _paged_inputs(oracle, dev, _base(171, B, S, D, (64,)), "flat", elem)
    assert x.lengths.min() == 0 and x.lengths.max() == S - 1
    ck = Checker("flat", elem)
    e_o, e_p = fm.attention_error(x.oracle[2], x.model), fm.probability_error(x.oracle[1], x.model)
    try:
        assert mli.mli_tune(b"scan_stream", 0) == 0
        got = {}
        for nt in (0, 1):
            assert mli.mli_tune(b"nt_loads", nt) == 0
            qkt = torch.full((B, S), SENTINEL, device=dev)
            out = torch.full((B, D), SENTINEL, device=dev)
            ops.decode_scan_paged(x.q, x.page_table, x.L, qkt, out, ELEM[elem], phases=3)
            ck.check(f"paged scan, materialising, nt_loads {nt}", "attention", fm.attention_error(host(out), x.model), e_o)
            ck.check(f"paged scan, materialising, nt_loads {nt}", "probabilities", fm.probability_error(host(qkt), x.model), e_p)
            lean = _lean_twice(ops, x, elem, f"lean, nt_loads {nt}")
            ck.check(f"paged scan, lean, nt_loads {nt}", "attention", fm.attention_error(lean, x.model), e_o)
            got[nt] = (host(out).copy(), host(qkt).copy(), lean)
        for a, b, what in zip(got[1], got[0], ("attention_result", "probabilities", "lean attention_result")):
            assert_equal(a, b, what=f"{elem} D {D} {what}: nt_loads 1 against nt_loads 0")
    finally:
        mli.mli_tune(b"scan_stream", 1)
        mli.mli_tune(b"nt_loads", 2)
    ck.done()


@pytest.mark.parametrize("D", [128, 1536])
def test_equal_page_shares_scan_under_both_cache_policies(oracle, mli, dev, D):
    """test_equal_page_shares_scan (9 rows of n_sequence 1024, the lengths of STREAM_CASES' emb_dim-1024 case) under nt_loads 0 and 1.
    There for the fp8 kernels no other judged case launches (tests/kernel_coverage.json):
      D 128:  fused_decode_stream_kernel<ElemFP8, 1, true, 2, 4, 4> (four token slots per load instruction, non-temporal);
      D 1536: fused_decode_stream_kernel<ElemFP8, 2, NT, 4, 2, 1> (two lane loads: emb_dim 1040 .. 2047 on fp8 pages; more than
              64 KiB of dynamic LDS).  fp32 and bf16 pages of that width take the chunked scan."""
    lengths = [0, 1023, 0, 0, 16, 17, 512, 1, 1008]
    try:
        for nt in (0, 1):
            assert mli.mli_tune(b"nt_loads", nt) == 0
            test_equal_page_shares_scan(oracle, mli, dev, 197, len(lengths), 1024, D, lengths, "flat")
    finally:
        mli.mli_tune(b"nt_loads", 2)


# ---- the fp32 compositions, from the inputs -------------------------------------------------------------------------------
# (seed, B, S, D): one chunk, several chunks, the long rows
COMPOSITION_SHAPES = [(151, 24, 64, 512), (153, 20, 1024, 256), (154, 18, 4096, 512), (155, 20, 256, 1024)]


def _composition_case(seed, B, S, D, family, with_new_rows):
    """Inputs of a composition in the given family.  q is projected from x[L - 1], so `peaked` scales wq, and the K edits of
    the other families use the float64 projection of q; rows listed as new have their whole K / V recomputed from x (flat
    there, whatever the family), every row's slot L - 1 is recomputed."""
    chunks = (64, 256) if S > 256 else (64,) if S > 64 else ()
    L = edge_lengths(seed, B, S, chunks)
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    # new rows (prefilled from x by the composition): a few short ones across the first chunk edges -- the CPU oracle's
    # prefill is O(L D^2) per row
    new = [b for b in range(B) if int(L[b]) in (2, 17, 63, 65, 257)] if with_new_rows else []
    c["n_new"] = len(new)
    c["new_batch_idx"][:len(new)] = new
    if family == "peaked":
        c["wq"] = (c["wq"] * np.float32(12.0)).astype(np.float32)
    q64, k64, v64, q_scale, _, _ = fm.project_latest(c["inp_embedding"], L, c["wk"], c["wq"], c["wv"])
    live = L > 0
    q_before = c["q_output"].copy()
    c["q_output"][live] = q64[live].astype(np.float32)         # (what the families derive the score direction from)
    _, c["kt_cache"] = apply_family(c, "flat" if family == "peaked" else family)
    # the float64 model of the caches after fill + latest
    kt = c["kt_cache"].astype(np.float64)
    v = c["v_cache"].astype(np.float64)
    for b in c["new_batch_idx"][:c["n_new"]]:
        n = int(L[b])
        x = c["inp_embedding"][b, :n].astype(np.float64)
        kt[b, :, :n] = (x @ c["wk"].astype(np.float64)).T
        v[b, :n] = x @ c["wv"].astype(np.float64)
    for b in np.nonzero(live)[0]:
        kt[b, :, L[b] - 1] = k64[b]
        v[b, L[b] - 1] = v64[b]
    model = fm.Model(q64, kt, v, L)
    model.q, model.q_scale = q64, q_scale
    poison_contiguous(c["q_output"], c["kt_cache"], c["v_cache"], L)
    model.q_poison = c["q_output"]                             # the direction the finite poison of the pages is built from
    c["q_output"] = q_before                                   # the compositions start from unrelated q_output contents
    return c, model


def _oracle_composition(oracle, c):
    o = {k: c[k].copy() for k in ("kt_cache", "v_cache", "q_output", "qkt_output", "attention_result")}
    oracle.self_attention_inference_host(c["inp_embedding"], c["lengths"], c["wk"], c["wq"], c["wv"], c["new_batch_idx"],
                                         o["kt_cache"], o["v_cache"], o["q_output"], o["qkt_output"], o["attention_result"],
                                         c["n_new"])
    return o


@pytest.mark.parametrize("with_new_rows", [False, True])
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("seed,B,S,D", COMPOSITION_SHAPES)
def test_fp32_compositions(oracle, mli, dev, seed, B, S, D, family, with_new_rows):
    """paged_attention, paged_attention_lean, inference_self_attention (softmax fused and not) and self_attention_lean:
    q_output and attention_result against project_latest + the model; tolerance from the oracle's composition."""
    from min_llm_inference_amd import ops
    c, m = _composition_case(seed, B, S, D, family, with_new_rows)
    L = c["lengths"]
    o = _oracle_composition(oracle, c)
    e_q = fm.projection_error(o["q_output"], m.q, L, m.q_scale)
    e_o = fm.attention_error(o["attention_result"], m)
    ck = Checker(family)

    def judge(path, d):
        ck.check(path, "q_output", fm.projection_error(host(d["q_output"]), m.q, L, m.q_scale), e_q)
        ck.check(path, "attention", fm.attention_error(host(d["attention_result"]), m), e_o)

    def contiguous():
        d = {k: _t(c[k], dev) for k in ("inp_embedding", "lengths", "wk", "wq", "wv", "new_batch_idx", "kt_cache", "v_cache",
                                        "q_output", "qkt_output")}
        d["attention_result"] = torch.full((B, D), SENTINEL, device=dev)
        return d

    def paged():
        # pages as the reference's wrapper fills them (slots s <= L), dead K / V slots finite poison
        values, _ = fill_pages(oracle, c, m.q_poison, c["kt_cache"], c["v_cache"], finite_poison=True)
        d = {k: _t(c[k], dev) for k in ("lengths", "wk", "wq", "wv", "new_batch_idx", "q_output", "qkt_output")}
        d["pool"] = _t(values, dev)
        d["page_table"] = _t(np.where(c["table"] >= 0, d["pool"].data_ptr() + 4 * c["table"], 0).astype(np.int64), dev)
        d["attention_result"] = torch.full((B, D), SENTINEL, device=dev)
        return d

    try:
        for fused in (1, 0):
            assert mli.mli_tune(b"fused_softmax", fused) == 0
            d = contiguous()
            ops.inference_self_attention(d["inp_embedding"], d["lengths"], d["wk"], d["wq"], d["wv"], d["new_batch_idx"],
                                         d["kt_cache"], d["v_cache"], d["q_output"], d["qkt_output"], d["attention_result"],
                                         c["n_new"])
            judge("inference_self_attention", d)
            d = paged()
            ops.paged_attention(d["page_table"], d["lengths"], d["wk"], d["wq"], d["wv"], d["new_batch_idx"], d["q_output"],
                                d["qkt_output"], d["attention_result"], c["n_new"], S)
            judge("paged_attention", d)
    finally:
        mli.mli_tune(b"fused_softmax", -1)
    d = contiguous()
    for _ in range(2):
        ops.self_attention_lean(d["inp_embedding"], d["lengths"], d["wk"], d["wq"], d["wv"], d["new_batch_idx"],
                                d["kt_cache"], d["v_cache"], d["q_output"], d["attention_result"], c["n_new"])
        judge("self_attention_lean", d)
    d = paged()
    for _ in range(2):
        ops.paged_attention_lean(d["page_table"], d["lengths"], d["wk"], d["wq"], d["wv"], d["new_batch_idx"], d["q_output"],
                                 d["attention_result"], c["n_new"], S)
        judge("paged_attention_lean", d)
    ck.done()


# ---- full size, on the timed path ----------------------------------------------------------------------------------------
def test_config4_bf16_lean_step_at_fp32_accuracy(oracle, mli, dev):
    """BASELINE config 4 (B = 1024, S = 4096, D = 512, bf16 pages) as bench.py builds and times it -- wl.lean_step(): projection,
    the equal-shares bf16 scan, decoder head -- on the >= 128 sampled rows of
    test_full_size_properties_gpu.test_config4_default_lean_step_matches_the_oracle_on_128_rows, attention_result under the
    condition-scaled metric in place of 1e-3 absolute.  The model reads what the step left in memory: the fp32 q_output and
    the bf16 K / V rows of the pages (the appended row included); dead slots are NaN."""
    import test_full_size_properties_gpu as fs
    wl = fs._workload("c4", dev, "bf16")
    try:
        fs._poison_dead_slots(wl)
        Lall = wl.lengths_host.astype(np.int64)
        cut, dyn = fs._share_boundary_rows(Lall)
        rows = {int(np.argmin(Lall)), int(np.argmax(Lall))}
        rows.update(int(b) for b in cut[:: max(1, len(cut) // 70)])
        rows.update(int(b) for b in dyn[:: max(1, len(dyn) // 24)])
        rows.update(range(0, wl.B, wl.B // 40))
        rows = sorted(rows)
        assert len(rows) >= 128, len(rows)
        wl.attention_result.fill_(-7.0)
        wl.lean_step()
        torch.cuda.synchronize()
        got = wl.attention_result.cpu().numpy()
        q = wl.q_output.cpu().numpy()
        assert np.isfinite(got).all()
        ck = Checker("bench state (lengths U[S/4, 3S/4])", "bf16")
        for i0 in range(0, len(rows), 32):
            part = rows[i0:i0 + 32]
            Lp = wl.lengths_host[part].astype(np.int32)     # the scan of the step reads rows of the length before the step
            k = torch.nan_to_num(fs._rows_from_pages(wl, part, 1)).cpu().numpy()
            v = torch.nan_to_num(fs._rows_from_pages(wl, part, 2)).cpu().numpy()
            ktm = k.transpose(0, 2, 1)
            m = fm.Model(q[part], ktm, v, Lp)
            _, _, o_or = oracle_scan(oracle, np.ascontiguousarray(q[part]), ktm, v, Lp)
            ck.check("lean_step at config 4 (equal-page-shares scan)", "attention", fm.attention_error(got[part], m),
                     fm.attention_error(o_or, m))
        ck.done()
    finally:
        del wl
        torch.cuda.empty_cache()
