"""BASELINE.json's FULL sizes on the GPU (config 3: B=256, S=1024, D=256 fp32; config 4: B=1024, S=4096, D=512,
bf16 pages) -- the state bench.py times (shuffled page pool, lengths U[S/4, 3S/4]).  The oracle still covers the
decode step of config 3 in full and a row sample of config 4; on top of that, properties that hold at any size:
probabilities sum to one with an exact zero tail, a row whose V rows are all equal returns that row, slots beyond a
row's length are never read (they are NaN here), chunking and the two forms of the composition agree, and a repeated
launch is bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

from helpers import assert_close, assert_equal

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAGE = 16


def _workload(name, dev, dtype):
    sys.path.insert(0, ROOT)
    import bench
    return bench.Workload(name, dev, 0xC0FFEE, headroom=8, dtype=dtype)


def _pool_view(wl):
    return wl.pool.view(-1, PAGE, 3, wl.D)


def _poison_dead_slots(wl):
    """NaN into every slot at or beyond its row's length (x, K and V): nothing there may reach a result."""
    pid = torch.from_numpy(wl.page_ids).to(wl.dev)                                  # [B, W]
    s = (torch.arange(wl.S // PAGE, device=wl.dev)[:, None] * PAGE + torch.arange(PAGE, device=wl.dev)[None, :])
    live = s[None, :, :] < wl.lengths[:, None, None]                                   # [B, W, 16]
    ok = pid >= 0
    dead = torch.ones(_pool_view(wl).shape[0], PAGE, dtype=torch.bool, device=wl.dev)
    dead[pid[ok]] = ~live[ok]
    _pool_view(wl)[dead] = float("nan")


def _rows_from_pages(wl, rows, seg):
    """[len(rows), S, D] fp32 copy of segment `seg` of the given batch rows (zeros where no page is allocated)."""
    out = torch.zeros(len(rows), wl.S, wl.D, device=wl.dev)
    pv = _pool_view(wl)
    lut = None
    if pv.dtype == torch.uint8:   # fp8 pages: OCP e4m3 codes, decoded through the numpy model's table
        from helpers import fp8_decode
        lut = torch.from_numpy(fp8_decode(np.arange(256, dtype=np.uint8))).to(wl.dev)
    for i, b in enumerate(rows):
        ids = wl.page_ids[b]
        n = int((ids >= 0).sum())
        raw = pv[torch.from_numpy(ids[:n]).to(wl.dev), :, seg, :].reshape(n * PAGE, wl.D)
        out[i, :n * PAGE] = raw.float() if lut is None else lut[raw.long()]
    return out


def _check_probabilities(wl, probs):
    L = wl.lengths
    mask = torch.arange(wl.S, device=wl.dev)[None, :] < L[:, None]
    assert torch.isfinite(probs).all()
    assert (probs >= 0).all()
    assert (probs[~mask] == 0).all(), "zero tail"
    sums = probs.sum(dim=1)
    assert torch.allclose(sums[L > 0], torch.ones_like(sums[L > 0]), atol=1e-4), (sums.min().item(), sums.max().item())


@pytest.fixture(scope="module")
def c4(dev, mli):
    wl = _workload("c4", dev, "bf16")
    _poison_dead_slots(wl)
    yield wl
    del wl
    torch.cuda.empty_cache()


def test_config4_step_probabilities_masking_and_oracle_sample(oracle, mli, c4):
    from min_llm_inference_amd import ops
    wl = c4
    rows = list(range(0, wl.B, wl.B // 32))[:32]                      # 32 rows spread over the batch
    x = _rows_from_pages(wl, rows, 0).cpu().numpy()
    ops.paged_attention_bf16(wl.page_table, wl.lengths, wl.wk, wl.wq, wl.wv, wl.new_idx, wl.q_output, wl.qkt_output,
                             wl.attention_result, 0, wl.S)
    torch.cuda.synchronize()
    _check_probabilities(wl, wl.qkt_output)
    assert torch.isfinite(wl.attention_result).all() and torch.isfinite(wl.q_output).all()
    # oracle on the sampled rows: bf16-rounded inputs, K / V as the pages hold them AFTER the step (bf16), fp32 math
    k = _rows_from_pages(wl, rows, 1).cpu().numpy()
    v = _rows_from_pages(wl, rows, 2).cpu().numpy()
    L = wl.lengths_host[rows].copy()
    for i in range(len(rows)):                                         # dead slots are NaN in the pages
        x[i, L[i]:] = 0; k[i, L[i]:] = 0; v[i, L[i]:] = 0
    wq = wl.wq.float().cpu().numpy()
    q = np.stack([x[i, L[i] - 1] @ wq for i in range(len(rows))]).astype(np.float32)
    assert_close(wl.q_output[rows].cpu().numpy(), q, what="q_output of the sampled rows")
    kt = np.ascontiguousarray(k.transpose(0, 2, 1))
    s = np.zeros((len(rows), wl.S), np.float32)
    o = np.zeros((len(rows), wl.D), np.float32)
    oracle.qkt_host(q, kt, L, s)
    oracle.softmax_in_place_with_lengths_host(s, L)
    oracle.softmax_v_host(s, v, o, L)
    assert_close(wl.qkt_output[rows].cpu().numpy(), s, what="probabilities of the sampled rows")
    assert_close(wl.attention_result[rows].cpu().numpy(), o, what="attention_result of the sampled rows")


def _share_boundary_rows(lengths, n_workgroups=512, dyn_pct=4, gran=64):
    """Rows of the equal-shares scan (attention_stream.hip) that are cut by a static share boundary, and rows that lie
    (partly) in the dynamic part handed out in granules: the rows whose result is a merge of several workgroups' triples."""
    pages = -(-np.asarray(lengths, np.int64) // PAGE)
    prefix = np.concatenate([[0], np.cumsum(pages)])
    P = int(prefix[-1])
    Ps = P - P * dyn_pct // 100 if dyn_pct > 0 and P * dyn_pct // 100 >= gran else P
    cuts = np.unique((np.arange(1, n_workgroups) * Ps) // n_workgroups)
    cut_rows = np.searchsorted(prefix, cuts, side="right") - 1          # row holding page index `cut`
    inside = cuts > prefix[cut_rows]                                      # boundary strictly inside the row
    dyn_rows = np.nonzero(prefix[1:] > Ps)[0]
    return np.unique(cut_rows[inside]), dyn_rows


def test_config4_default_lean_step_matches_the_oracle_on_128_rows(oracle, mli, c4):
    """What bench.py times at config 4 -- wl.lean_step(): projection, the EQUAL-SHARES bf16 scan
    (fused_decode_stream_kernel<ElemBF16, ...>, the kernel `roofline` is quoted on), fused decoder head -- against the
    oracle directly: >= 128 rows including the shortest and the longest row, rows cut by a share boundary and rows of
    the dynamically distributed tail.  Oracle inputs are what the pages hold (bf16 x, K, V; the row's newest K / V as
    the oracle computes them from x, rounded to bf16 like the page stores them); all arithmetic fp32."""
    from helpers import bf16_round
    wl = c4
    L = wl.lengths_host.astype(np.int64)
    cut, dyn = _share_boundary_rows(L)
    assert len(cut) >= 64 and len(dyn) >= 8
    rows = {int(np.argmin(L)), int(np.argmax(L))}
    rows.update(int(b) for b in cut[:: max(1, len(cut) // 70)])
    rows.update(int(b) for b in dyn[:: max(1, len(dyn) // 24)])
    rows.update(range(0, wl.B, wl.B // 40))
    rows = sorted(rows)
    assert len(rows) >= 128, len(rows)
    saved = wl.lengths.clone()
    try:
        wl.attention_result.fill_(-7.0)
        wl.lean_step()
        torch.cuda.synchronize()
        got = wl.attention_result.cpu().numpy()
        got_q = wl.q_output.cpu().numpy()
        tok = wl.decoder_result.view(-1).cpu().numpy()
        assert (wl.lengths.cpu().numpy() == wl.lengths_host + 1).all()
    finally:
        wl.lengths.copy_(saved)
    w = [t.float().cpu().numpy() for t in (wl.wk, wl.wq, wl.wv)]
    emb = wl.emb_table.cpu().numpy()
    worst = 0.0
    for i0 in range(0, len(rows), 32):                                  # 32 rows at a time: 3 x 256 MiB of host copies
        part = rows[i0:i0 + 32]
        x = _rows_from_pages(wl, part, 0).cpu().numpy()
        k = _rows_from_pages(wl, part, 1).cpu().numpy()
        v = _rows_from_pages(wl, part, 2).cpu().numpy()
        Lp = wl.lengths_host[part].copy()
        for i in range(len(part)):                                      # dead slots are NaN in the pages
            x[i, Lp[i]:] = 0; k[i, Lp[i]:] = 0; v[i, Lp[i]:] = 0
        kt = np.ascontiguousarray(k.transpose(0, 2, 1))
        q = np.zeros((len(part), wl.D), np.float32)
        oracle.get_latest_kt_q_v(x, Lp, w[0], w[1], w[2], kt, v, q)     # the oracle's own projection of x[L-1]
        idx = np.arange(len(part))
        # ... agrees with what the step left in the pages (bf16: half an ulp of the page element) and is stored as the page stores it
        assert_close(k[idx, Lp - 1], kt[idx, :, Lp - 1], thr=5e-3, what="appended K rows vs oracle projection")
        kt[idx, :, Lp - 1] = bf16_round(kt[idx, :, Lp - 1])
        v[idx, Lp - 1] = bf16_round(v[idx, Lp - 1])
        assert_close(got_q[part], q, what="q_output")
        sc = np.zeros((len(part), wl.S), np.float32)
        o = np.zeros((len(part), wl.D), np.float32)
        oracle.qkt_host(q, kt, Lp, sc)
        oracle.softmax_in_place_with_lengths_host(sc, Lp)
        oracle.softmax_v_host(sc, v, o, Lp)
        # bf16 is unpinned by the reference; the bar here is the fp32 one, 1e-3, except that an appended K / V
        # element may round to the other bf16 neighbour than the oracle's (different fp32 summation order in the MFMA):
        # one element of one of ~2000 rows, weighted by its probability -- far below 1e-3
        assert_close(got[part], o, what="attention_result of the default lean step vs oracle")
        worst = max(worst, float(np.abs(got[part] - o).max()))
        logits = oracle.gemm_transpose_host(np.ascontiguousarray(o), emb)
        best = logits.max(axis=1)
        assert (logits[idx, tok[part]] >= best - 1e-3).all(), "decoder token = an argmax of the oracle's logits (1e-3)"
    assert worst < 1e-3


def test_config4_fp8_lean_step_matches_the_oracle_on_128_rows(oracle, mli, dev):
    """BASELINE config 4's shape with fp8 (OCP e4m3) pages -- the opt-in extension bench.py reports as configs.c4_fp8: the
    lean step (projection from fp8 x rows, equal-shares scan with two token slots per load instruction, fused decoder
    head) against the oracle on >= 128 rows (shortest, longest, rows cut by share boundaries).  Dead K / V slots are NaN
    bytes (0x7f).  Unpinned by the reference (fp32 only): the oracle runs in fp32 on what the pages hold."""
    from helpers import fp8_round
    wl = _workload("c4", dev, "fp8")
    try:
        pid = torch.from_numpy(wl.page_ids).to(wl.dev)
        s = (torch.arange(wl.S // PAGE, device=wl.dev)[:, None] * PAGE + torch.arange(PAGE, device=wl.dev)[None, :])
        live = s[None, :, :] < wl.lengths[:, None, None]
        ok = pid >= 0
        dead = torch.ones(_pool_view(wl).shape[0], PAGE, dtype=torch.bool, device=wl.dev)
        dead[pid[ok]] = ~live[ok]
        _pool_view(wl)[:, :, 1:, :][dead] = 0x7f                              # K and V of every dead slot: NaN
        L = wl.lengths_host.astype(np.int64)
        cut, dyn = _share_boundary_rows(L)
        rows = {int(np.argmin(L)), int(np.argmax(L))}
        rows.update(int(b) for b in cut[:: max(1, len(cut) // 70)])
        rows.update(int(b) for b in dyn[:: max(1, len(dyn) // 24)])
        rows.update(range(0, wl.B, wl.B // 40))
        rows = sorted(rows)
        assert len(rows) >= 128
        wl.attention_result.fill_(-7.0)
        wl.lean_step()
        torch.cuda.synchronize()
        got = wl.attention_result.cpu().numpy()
        got_q = wl.q_output.cpu().numpy()
        tok = wl.decoder_result.view(-1).cpu().numpy()
        assert np.isfinite(got).all()
        assert (wl.lengths.cpu().numpy() == wl.lengths_host + 1).all()
        w = [t.float().cpu().numpy() for t in (wl.wk, wl.wq, wl.wv)]
        emb = wl.emb_table.cpu().numpy()
        for i0 in range(0, len(rows), 32):
            part = rows[i0:i0 + 32]
            x = _rows_from_pages(wl, part, 0).cpu().numpy()
            k = _rows_from_pages(wl, part, 1).cpu().numpy()
            v = _rows_from_pages(wl, part, 2).cpu().numpy()
            Lp = wl.lengths_host[part].copy()
            for i in range(len(part)):
                x[i, Lp[i]:] = 0; k[i, Lp[i]:] = 0; v[i, Lp[i]:] = 0
            kt = np.ascontiguousarray(k.transpose(0, 2, 1))
            q = np.zeros((len(part), wl.D), np.float32)
            oracle.get_latest_kt_q_v(x, Lp, w[0], w[1], w[2], kt, v, q)
            idx = np.arange(len(part))
            # the appended rows: what the step stored is the oracle's projection up to one fp8 step (2^-3 relative)
            assert_close(k[idx, Lp - 1], fp8_round(kt[idx, :, Lp - 1]), thr=0.13, what="appended K rows vs oracle projection")
            kt[idx, :, Lp - 1] = k[idx, Lp - 1]                                # the scan reads what the GPU stored
            v[idx, Lp - 1] = _rows_from_pages(wl, part, 2).cpu().numpy()[idx, Lp - 1]
            assert_close(got_q[part], q, what="q_output")
            sc = np.zeros((len(part), wl.S), np.float32)
            o = np.zeros((len(part), wl.D), np.float32)
            oracle.qkt_host(q, kt, Lp, sc)
            oracle.softmax_in_place_with_lengths_host(sc, Lp)
            oracle.softmax_v_host(sc, v, o, Lp)
            assert_close(got[part], o, what="attention_result of the fp8 lean step vs oracle")
            logits = oracle.gemm_transpose_host(np.ascontiguousarray(o), emb)
            best = logits.max(axis=1)
            assert (logits[idx, tok[part]] >= best - 1e-3).all(), "decoder token = an argmax of the oracle's logits (1e-3)"
    finally:
        del wl
        torch.cuda.empty_cache()


def test_config4_repeat_is_bit_identical_and_forms_agree(mli, c4):
    from min_llm_inference_amd import ops
    wl = c4

    def scan():
        ops.decode_scan_paged(wl.q_output, wl.page_table, wl.lengths, wl.qkt_output, wl.attention_result, True)
        torch.cuda.synchronize()
        return wl.qkt_output.clone(), wl.attention_result.clone()

    p0, o0 = scan()
    p1, o1 = scan()
    assert torch.equal(p0, p1) and torch.equal(o0, o1), "same launch twice: bit-identical"
    try:
        for ct in (256, 1024):                                     # other split points, other merge trees
            assert mli.mli_tune(b"chunk_tokens", ct) == 0
            p, o = scan()
            assert (p - p0).abs().max().item() <= 1e-6 and (o - o0).abs().max().item() <= 1e-5, ct
    finally:
        mli.mli_tune(b"chunk_tokens", 0)
    # the three-kernel form of the same block (q.K^T, masked softmax, softmax.V)
    ops.launch_qkt_paged_attention_bf16(wl.q_output, wl.page_table, wl.lengths, wl.qkt_output)
    ops.launch_softmax_in_place_with_lengths(wl.qkt_output, wl.lengths)
    ops.launch_softmax_v_paged_attention_bf16(wl.qkt_output, wl.page_table, wl.attention_result, wl.lengths)
    torch.cuda.synchronize()
    assert (wl.qkt_output - p0).abs().max().item() <= 1e-6
    assert (wl.attention_result - o0).abs().max().item() <= 1e-5


def test_config4_lean_scan_equals_materialising_under_full_load(mli, c4):
    """The in-kernel merge is a hand-off between workgroups (write-through partials, arrival counter, acquire): it has
    to hold with every CU streaming and ragged rows finishing at different times, and on repeated launches (the
    consumer's caches warm with the previous launch's lines at the same addresses).  Every word of attention_result is
    compared, bit for bit, with the two-launch form -- also with lengths that change between launches as they do in a
    running engine."""
    from min_llm_inference_amd import ops
    wl = c4
    saved = wl.lengths.clone()

    def full():
        ops.decode_scan_paged(wl.q_output, wl.page_table, wl.lengths, wl.qkt_output, wl.attention_result, True)
        torch.cuda.synchronize()
        return wl.attention_result.clone()

    def lean():
        wl.attention_result.fill_(-7.0)
        ops.decode_scan_paged(wl.q_output, wl.page_table, wl.lengths, None, wl.attention_result, True, phases=7,
                              n_sequence=wl.S)
        torch.cuda.synchronize()
        return wl.attention_result.clone()

    try:
        ref = full()
        # default lean form at this size: equal page shares (attention_stream.hip) -- other split points of a row than the
        # chunked grid, so other fp32 roundings in the merge; the same bits on every launch
        first = lean()
        assert (first - ref).abs().max().item() <= 1e-5
        for _ in range(4):
            assert torch.equal(lean(), first)
        assert mli.mli_tune(b"scan_stream", 0) == 0     # the chunked lean form: bit-identical to the two-launch form
        for _ in range(4):
            assert torch.equal(lean(), ref)
        g = torch.Generator(device=wl.dev)
        g.manual_seed(5)
        for _ in range(3):                                           # shorter rows: other chunk counts per row
            wl.lengths.copy_((saved.float() * torch.rand(wl.B, device=wl.dev, generator=g)).int().clamp_(min=0))
            wl.lengths[::97] = 0
            want = full()
            assert torch.equal(lean(), want)
            mli.mli_tune(b"scan_stream", 1)                          # ... and other shares per workgroup
            got = lean()
            assert (got - want).abs().max().item() <= 1e-5 and torch.equal(lean(), got)
            assert (got[::97] == 0).all()
            mli.mli_tune(b"scan_stream", 0)
    finally:
        mli.mli_tune(b"scan_stream", 1)
        wl.lengths.copy_(saved)


def test_config4_rows_of_equal_v_return_that_row(mli, c4):
    """softmax weights sum to one, so a row whose live V rows all equal c gives c (bf16 c, fp32 accumulation)."""
    from min_llm_inference_amd import ops
    wl = c4
    pv = _pool_view(wl)
    c = (torch.rand(wl.B, wl.D, device=wl.dev) * 2 - 1).to(pv.dtype)
    pid = torch.from_numpy(wl.page_ids).to(wl.dev)
    for b0 in range(0, wl.B, 64):                                   # V segment of every allocated page of the row := c_b
        ids = pid[b0:b0 + 64]
        ok = ids >= 0
        rows = torch.arange(b0, min(b0 + 64, wl.B), device=wl.dev)[:, None].expand_as(ids)[ok]
        pv[ids[ok], :, 2, :] = c[rows][:, None, :].expand(-1, PAGE, -1)
    ops.decode_scan_paged(wl.q_output, wl.page_table, wl.lengths, wl.qkt_output, wl.attention_result, True)
    torch.cuda.synchronize()
    err = (wl.attention_result - c.float()).abs().max().item()
    assert err <= 2e-4, err


def test_config3_full_size_step_matches_the_oracle(oracle, mli, dev):
    from min_llm_inference_amd import ops
    wl = _workload("c3", dev, "f32")
    _poison_dead_slots(wl)
    rows = list(range(wl.B))
    x = _rows_from_pages(wl, rows, 0).cpu().numpy()
    k = _rows_from_pages(wl, rows, 1).cpu().numpy()
    v = _rows_from_pages(wl, rows, 2).cpu().numpy()
    L = wl.lengths_host.copy()
    for b in rows:
        x[b, L[b]:] = 0; k[b, L[b]:] = 0; v[b, L[b]:] = 0
    ops.paged_attention(wl.page_table, wl.lengths, wl.wk, wl.wq, wl.wv, wl.new_idx, wl.q_output, wl.qkt_output,
                        wl.attention_result, 0, wl.S)
    torch.cuda.synchronize()
    _check_probabilities(wl, wl.qkt_output)
    kt = np.ascontiguousarray(k.transpose(0, 2, 1))
    q = np.zeros((wl.B, wl.D), np.float32)
    s = np.zeros((wl.B, wl.S), np.float32)
    o = np.zeros((wl.B, wl.D), np.float32)
    w = [t.cpu().numpy() for t in (wl.wk, wl.wq, wl.wv)]
    oracle.self_attention_inference_host(x, L, w[0], w[1], w[2], np.zeros((wl.B,), np.int32), kt, v, q, s, o, 0)
    assert_close(wl.q_output.cpu().numpy(), q, what="q_output")
    assert_close(wl.qkt_output.cpu().numpy(), s, what="probabilities")
    assert_close(wl.attention_result.cpu().numpy(), o, what="attention_result")
    # the K / V rows appended by the step, through the page layout
    k_after = _rows_from_pages(wl, rows, 1).cpu().numpy()
    v_after = _rows_from_pages(wl, rows, 2).cpu().numpy()
    idx = np.arange(wl.B)
    assert_close(k_after[idx, L - 1], kt[idx, :, L - 1], what="appended K rows")
    assert_close(v_after[idx, L - 1], v[idx, L - 1], what="appended V rows")
    # the lean one-call step (what bench.py times at config 3: panel projection, chunked lean scan with the in-kernel
    # merge, fused decoder head) from the same state, against the oracle directly
    first = wl.attention_result.clone()
    wl.attention_result.fill_(-7.0)
    wl.q_output.fill_(-7.0)
    wl.lean_step()
    torch.cuda.synchronize()
    assert torch.equal(wl.attention_result, first), "lean == materialising, bit for bit (chunked grid)"
    assert_close(wl.q_output.cpu().numpy(), q, what="q_output of the lean step")
    assert_close(wl.attention_result.cpu().numpy(), o, what="attention_result of the lean step")
    tok = wl.decoder_result.view(-1).cpu().numpy()
    logits = oracle.gemm_transpose_host(o, wl.emb_table.cpu().numpy())
    best = logits.max(axis=1)
    assert (logits[idx, tok] >= best - 1e-3).all(), "decoder token = an argmax of the oracle's logits (1e-3)"
    assert (wl.lengths.cpu().numpy() == L + 1).all()


def test_config2_full_size_step_matches_the_oracle(oracle, mli, dev):
    """BASELINE config 2 at its full size (B=256, D=256, S=1024, contiguous caches, fp32): one decode step -- the
    materialising composition and the lean one-call step -- against the oracle on every row; slots at or beyond a row's
    length are NaN in all three caches and must never reach a result."""
    from min_llm_inference_amd import ops
    wl = _workload("c2", dev, "f32")
    L = wl.lengths_host.copy()
    s = torch.arange(wl.S, device=wl.dev)
    dead = s[None, :] >= wl.lengths[:, None]                                    # [B, S]
    wl.inp_embedding[dead] = float("nan")
    wl.v_cache[dead] = float("nan")
    wl.kt_cache.transpose(1, 2)[dead] = float("nan")
    x = torch.nan_to_num(wl.inp_embedding).cpu().numpy()
    kt = torch.nan_to_num(wl.kt_cache).cpu().numpy()
    v = torch.nan_to_num(wl.v_cache).cpu().numpy()
    kt0, v0 = wl.kt_cache.clone(), wl.v_cache.clone()
    ops.inference_self_attention(wl.inp_embedding, wl.lengths, wl.wk, wl.wq, wl.wv, wl.new_idx, wl.kt_cache, wl.v_cache,
                                 wl.q_output, wl.qkt_output, wl.attention_result, 0)
    torch.cuda.synchronize()
    _check_probabilities(wl, wl.qkt_output)
    q = np.zeros((wl.B, wl.D), np.float32)
    sc = np.zeros((wl.B, wl.S), np.float32)
    o = np.zeros((wl.B, wl.D), np.float32)
    w = [t.cpu().numpy() for t in (wl.wk, wl.wq, wl.wv)]
    oracle.self_attention_inference_host(x, L, w[0], w[1], w[2], np.zeros((wl.B,), np.int32), kt, v, q, sc, o, 0)
    assert_close(wl.q_output.cpu().numpy(), q, what="q_output")
    assert_close(wl.qkt_output.cpu().numpy(), sc, what="probabilities")
    assert_close(wl.attention_result.cpu().numpy(), o, what="attention_result")
    idx = np.arange(wl.B)
    assert_close(wl.kt_cache.cpu().numpy()[idx, :, L - 1], kt[idx, :, L - 1], what="appended K columns")
    assert_close(wl.v_cache.cpu().numpy()[idx, L - 1], v[idx, L - 1], what="appended V rows")
    # the lean one-call step (what bench.py times) from the same state: same attention_result, then the decoder head
    first = wl.attention_result.clone()
    wl.kt_cache.copy_(kt0); wl.v_cache.copy_(v0)
    wl.attention_result.zero_()
    wl.lean_step()
    torch.cuda.synchronize()
    # (the lean composition keeps the probabilities in LDS and merges 256-token chunks: fp32 rounding of the merge apart)
    assert_close(wl.attention_result.cpu().numpy(), first.cpu().numpy(), thr=2e-5, what="lean vs materialising")
    assert_close(wl.attention_result.cpu().numpy(), o, what="attention_result of the lean step")
    tok = wl.decoder_result.view(-1).cpu().numpy()
    logits = o @ wl.emb_table.cpu().numpy().T
    best = logits.max(axis=1)
    assert (logits[idx, tok] >= best - 1e-3).all(), "decoder token = an argmax of the oracle's logits (1e-3)"
    assert (wl.lengths.cpu().numpy() == L + 1).all()


def test_config2_lean_scan_repeated_launches_with_changing_lengths(mli, dev):
    """The contiguous single-launch scan at config 2's size, 40 launches back to back with fresh random lengths each
    time (empty rows, single tokens, chunk boundaries, full rows), each against the three-launch composition on the same
    state: the rows' in-kernel merges (arrival counters, write-through partial rows) under load."""
    from min_llm_inference_amd import ops
    wl = _workload("c2", dev, "f32")
    rng = np.random.default_rng(20260)
    want = torch.empty_like(wl.attention_result)
    wl.q_output.copy_(torch.rand(wl.B, wl.D, device=dev) * 2 - 1)
    special = np.array([0, 1, 255, 256, 257, 512, 513, 1023, 1024], np.int32)
    for it in range(40):
        L = rng.integers(0, wl.S + 1, size=wl.B).astype(np.int32)
        L[rng.integers(0, wl.B, size=len(special))] = special
        wl.lengths.copy_(torch.from_numpy(L).to(dev))
        ops.launch_qkt(wl.q_output, wl.kt_cache, wl.lengths, wl.qkt_output)
        ops.launch_softmax_in_place_with_lengths(wl.qkt_output, wl.lengths)
        ops.launch_softmax_v(wl.qkt_output, wl.v_cache, want, wl.lengths)
        wl.attention_result.fill_(7.0)
        ops.decode_scan_contiguous(wl.q_output, wl.kt_cache, wl.v_cache, wl.lengths, wl.attention_result)
        torch.cuda.synchronize()
        assert_close(wl.attention_result.cpu().numpy(), want.cpu().numpy(), thr=2e-5, what=f"launch {it}")
