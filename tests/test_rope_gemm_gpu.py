"""The projection and the fills with rotary position embeddings (mli_get_latest_k_q_v_paged_rope,
mli_fill_new_k_v_cache_paged_rope, mli_paged_prefill_rope) on the GPU, every kernel form forced by its mli_tune key with the
launch counters as witness.  The whole pool and q_output are compared, so unwritten bytes count.  On every case:
  (a) the float64 judge of tests/rope_model.py passes (tests/test_rope_model_cpu.py proves that it can fail);
  (b) a table of all (1, 0) gives the bytes of the un-rotated entry point in the whole pool and in q_output -- that entry
      point run on the same tiled form (the panel and LDS-DMA kernels, which a table routes around, switched off for it);
  (c) with the standard table V, x and every row at slot 0 keep those bytes, while K and q differ elsewhere.
An fp32 emb_dim of 66 is refused by every paged entry point (tests/test_rope_abi.py); the scalar-load form runs at emb_dim 68
with weights that are not 16-byte aligned."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import gemm_model as gm
import rope_model as rp
from gpu_util import host
from test_gemm_edges_gpu import DEFAULTS, _shifted, _t

pytestmark = pytest.mark.gpu

KNOB = {"fc": b"fill_compact", "lc": b"latest_compact", "split": b"gemm_split", "pf": b"prefill_fused", "panel": b"gemm_panel",
        "tall": b"gemm_tall_tiles", "native": b"bf16_native_mfma", "dma": b"gemm_bf16_split"}
TILED = {"panel": 0, "dma": 0}      # the un-rotated reference of (b): the tiled kernels, as with a table


@contextlib.contextmanager
def tuned(mli, knobs):
    try:
        for k, v in knobs.items():
            assert mli.mli_tune(KNOB[k], v) == 0, k
        yield
    finally:
        for k, v in DEFAULTS.items():
            mli.mli_tune(k, v)


def _count(mli, family):
    n = ctypes.c_ulonglong(0)
    assert mli.mli_launch_count(family.encode(), ctypes.byref(n)) == 0
    return n.value


def _weights(c, dev, shift):
    if c.fmt == "f32":
        return {n: (_shifted(w, dev) if shift else _t(w, dev)) for n, w in c.w.items()}
    return {n: _t(gm.encode(w, "bf16"), dev) for n, w in c.w.items()}


def _spare_block(c):
    block = gm.PAGE * 3 * c.Din
    used = set((c.table[c.table >= 0] // block).tolist())
    return next(i for i in range(c.pool.size // block) if i not in used) * block


def _call(mli, dev, c, mode, H, knobs, table, W=0, K=0, shift=False):
    """One call on a fresh copy of the case's memory: table None = the un-rotated entry point.  Returns (pool, q) on the host."""
    from min_llm_inference_amd import ops
    fmt, elem = c.fmt, gm.ELEM[c.fmt]
    w = _weights(c, dev, shift)
    L, new_idx, q = _t(c.L, dev), _t(c.new_idx, dev), _t(c.q, dev)
    pool = _t(c.pool, dev)
    offsets = c.table.copy()
    if W:   # the table entry of a dead page names the spare page: it is never followed, and the spare page keeps its bytes
        spare = _spare_block(c)
        for b in range(c.B):
            for i in range(offsets.shape[1]):
                if offsets[b, i] >= 0 and rp.page_dead(i, int(c.L[b]), W, K):
                    offsets[b, i] = spare
    ptrs = _t(np.where(offsets >= 0, pool.data_ptr() + gm.ESIZE[fmt] * offsets, 0).astype(np.int64), dev)
    rope = None if table is None else _t(table, dev)
    kw = {} if table is None else dict(n_heads=H, rope=rope)
    with tuned(mli, knobs):
        if mode == "latest":
            ops.get_latest_k_q_v_paged_lean(ptrs, L, w["wk"], w["wq"], w["wv"], q, c.S, elem=elem, **kw)
        elif mode == "fill" and fmt == "fp8":   # fp8 pages have no fill entry point without the table: the lean composition
            out = torch.zeros(c.B, c.Din, device=dev)
            ops.paged_attention_lean(ptrs, L, w["wk"], w["wq"], w["wv"], new_idx, q, out, c.n_new, c.S, elem=elem,
                                     **({} if table is None else dict(n_heads=1, rope=rope)))
        elif mode == "fill" and table is None:
            fn = ops.launch_fill_new_k_v_cache_paged_attention if fmt == "f32" else ops.launch_fill_new_k_v_cache_paged_attention_bf16
            fn(ptrs, new_idx, L, w["wk"], w["wv"], c.n_new, c.S)
        elif mode == "fill":
            ops.fill_new_k_v_cache_paged_rope(ptrs, new_idx, L, w["wk"], w["wv"], c.n_new, c.S, H, rope, elem=elem)
        else:
            win = dict(window=W, sinks=K) if W else {}
            ops.paged_prefill(_t(c.emb, dev), _t(c.wpe, dev), _t(c.tok, dev), ptrs, L, new_idx, w["wk"], w["wv"], c.n_new, elem=elem,
                              **win, **kw)
    torch.cuda.synchronize()
    assert (host(L) == c.L).all() and (host(new_idx) == c.new_idx).all()
    p = host(pool)
    return (p.view(gm.BITS[fmt]) if fmt == "bf16" else p), host(q).copy()


def _check(oracle, mli, dev, label, c, mode, H, knobs, families, W=0, K=0, shift=False, library_table=False):
    """library_table: rotate by the table mli_rope_table writes (held to rope_model's restatement within an ulp of 1 here,
    bit for bit in tests/test_rope_abi.py where the two libms agree) instead of the restatement"""
    fmt = c.fmt
    composition = mode == "fill" and fmt == "fp8"
    Hc = 1 if composition else H
    std, ident = rp.standard_table(c.S, c.Din // Hc), rp.identity_table(c.S, c.Din // Hc)
    if library_table:
        from min_llm_inference_amd import ops
        lib_table = ops.rope_table(c.S, c.Din // Hc, 10000.0)
        assert lib_table.shape == std.shape and np.abs(lib_table.astype(np.float64) - std).max() <= 2.0 ** -23
        std = lib_table
    assert mli.mli_launch_counts_reset() == 0
    pool, q = _call(mli, dev, c, mode, Hc, knobs, std, W, K, shift)
    rope_family = "gemm_f32_rope" if fmt == "f32" or knobs.get("native") == 0 else "gemm_bf16_rope"
    counts = {f: _count(mli, f) for f in families + (rope_family, "gemm_f32_panel", "gemm_bf16_dma")}
    print(f"ROPE {label}: launches {counts}")
    assert counts["gemm_f32_panel"] == 0 and counts["gemm_bf16_dma"] == 0, counts
    assert counts[rope_family] == (2 if composition else 1), counts
    for f in families:
        assert counts[f] >= 1, (f, counts)
    # (a) the float64 judge
    fig = gm.Figures(label)
    e = rp.Expect(oracle, c, mode, std, Hc, W, K)
    if composition:   # fill, then latest: both judged, each leaving the other's slots alone
        e2 = rp.Expect(oracle, c, "latest", std, Hc)
        rp.judge(fig, c, e2, {"pool": pool}, q, also=e.rows)
        rp.judge(fig, c, e, {"pool": pool}, None, also=e2.rows)
    else:
        rp.judge(fig, c, e, {"pool": pool}, q if mode == "latest" else None)
        if mode != "latest":
            assert (q.view(np.uint32) == c.q.view(np.uint32)).all(), "a fill wrote q_output"
    fig.done()
    # (b) the identity table against the un-rotated entry point
    pool_i, q_i = _call(mli, dev, c, mode, Hc, knobs, ident, W, K, shift)
    pool_u, q_u = _call(mli, dev, c, mode, Hc, dict(knobs, **TILED), None, W, K, shift)
    bad = np.flatnonzero(gm.raw_bits(pool_i, fmt) != gm.raw_bits(pool_u, fmt))
    assert bad.size == 0, f"{label}: identity table: {bad.size} pool elements differ from the un-rotated call, first at {bad[0]}"
    assert (q_i.view(np.uint32) == q_u.view(np.uint32)).all(), f"{label}: identity table: q_output differs from the un-rotated call"
    assert (gm.raw_bits(pool_u, fmt) != gm.raw_bits(c.pool, fmt)).any(), "the un-rotated call wrote nothing"
    # (c) the standard table: V, x and slot 0 keep those bytes; K and q differ elsewhere
    rows = e.rows + (e2.rows if composition else [])
    k_off = gm._slot_offsets(c, rows, 1) if rows else np.zeros((0, c.Din), np.int64)
    moved = np.array([s > 0 for _, s in rows], bool)
    same = gm.raw_bits(pool, fmt) == gm.raw_bits(pool_u, fmt)
    rest = np.ones(c.pool.size, bool)
    rest[k_off[moved].ravel()] = False
    assert same[rest].all(), f"{label}: {int((~same[rest]).sum()) } elements outside the K rows of slots > 0 differ from the un-rotated call"
    assert moved.any() and not same[k_off[moved]].all(axis=1).any(), f"{label}: a K row at a slot > 0 kept its un-rotated bytes"
    if mode == "latest" or composition:
        live = np.array([b for b in range(c.B) if c.L[b] > 1], np.int64)
        at0 = np.array([b for b in range(c.B) if c.L[b] <= 1], np.int64)
        qs = q.view(np.uint32) == q_u.view(np.uint32)
        assert qs[at0].all(), f"{label}: q of a row at slot 0 (or empty) differs from the un-rotated call"
        assert len(live) and not qs[live].all(axis=1).any(), f"{label}: a q row at a slot > 0 kept its un-rotated bytes"


# ---- the decode projection ---------------------------------------------------------------------------------------------------------
def _latest_case(seed, fmt, B, S, D, small=False):
    rng = np.random.default_rng(seed)
    L = rng.integers(1, (8 if small else S) + 1, size=B).astype(np.int32)
    L[:10] = [0, 1, 16, 17, S, 0, 2, S - 1, 15, 33]
    return gm.Case(seed, "paged", fmt, "signed", B, S, D, D, L)


R64 = {"tall": 0, "split": 0, "lc": 0}
LATEST = [
    # id, fmt, D, H, knobs, families, shifted weights
    ("f32-rows64-D128-H1", "f32", 128, 1, R64, ("gemm_f32_rows64",), False),
    ("f32-rows64-D128-H2", "f32", 128, 2, R64, ("gemm_f32_rows64",), False),
    ("f32-rows64-D128-H4", "f32", 128, 4, R64, ("gemm_f32_rows64",), False),
    ("f32-panel-shape-D128-H4", "f32", 128, 4, {}, ("gemm_f32_rows64",), False),
    ("f32-rows64-compact-D128-H4", "f32", 128, 4, dict(R64, lc=2), ("gemm_f32_rows64", "latest_compact"), False),
    ("f32-rows128-D128-H2", "f32", 128, 2, {"tall": 2, "lc": 0}, ("gemm_f32_rows128",), False),
    ("f32-rows128-compact-D128-H4", "f32", 128, 4, {"tall": 2, "lc": 2}, ("gemm_f32_rows128", "latest_compact"), False),
    ("f32-split-D256-H4", "f32", 256, 4, {"tall": 0, "split": 1, "lc": 0}, ("gemm_f32_rows64_split",), False),
    ("f32-split-compact-D256-H4", "f32", 256, 4, {"tall": 0, "split": 1, "lc": 2}, ("gemm_f32_rows64_split", "latest_compact"), False),
    ("f32-scalar-loads-D68-H1", "f32", 68, 1, R64, ("gemm_f32_rows64",), True),
    ("f32-scalar-loads-D68-H2", "f32", 68, 2, dict(R64, lc=2), ("gemm_f32_rows64", "latest_compact"), True),
    ("bf16-rows64-D128-H1", "bf16", 128, 1, {"tall": 0, "lc": 0}, ("gemm_bf16_rows64",), False),
    ("bf16-rows64-D128-H2", "bf16", 128, 2, {"tall": 0, "lc": 2}, ("gemm_bf16_rows64", "latest_compact"), False),
    ("bf16-rows64-D128-H4", "bf16", 128, 4, {"tall": 0, "lc": 0}, ("gemm_bf16_rows64",), False),
    ("bf16-rows128-D128-H4", "bf16", 128, 4, {"tall": 2, "lc": 0}, ("gemm_bf16_rows128",), False),
    ("bf16-deep-D256-H4", "bf16", 256, 4, {"tall": 0, "lc": 0}, ("gemm_bf16_deep",), False),
    ("bf16-deep-compact-D256-H4", "bf16", 256, 4, {"tall": 0, "lc": 2}, ("gemm_bf16_deep", "latest_compact"), False),
    ("bf16-widened-D128-H4", "bf16", 128, 4, {"native": 0, "lc": 0}, ("gemm_bf16_widened",), False),
    ("bf16-widened-compact-D256-H4", "bf16", 256, 4, {"native": 0, "lc": 2}, ("gemm_bf16_widened", "latest_compact"), False),
    ("fp8-rows64-D128-H1", "fp8", 128, 1, {"tall": 0, "lc": 0}, ("gemm_bf16_rows64",), False),
    ("fp8-rows64-D128-H2", "fp8", 128, 2, {"tall": 0, "lc": 2}, ("gemm_bf16_rows64", "latest_compact"), False),
    ("fp8-rows64-D128-H4", "fp8", 128, 4, {"tall": 0, "lc": 0}, ("gemm_bf16_rows64",), False),
    ("fp8-rows128-D128-H4", "fp8", 128, 4, {"tall": 2, "lc": 0}, ("gemm_bf16_rows128",), False),
    ("fp8-deep-D256-H4", "fp8", 256, 4, {"tall": 0, "lc": 0}, ("gemm_bf16_deep",), False),
]


@pytest.mark.parametrize("fmt,D,H,knobs,families,shift", [pytest.param(*c[1:], id=c[0]) for c in LATEST])
def test_latest_projection(oracle, mli, dev, request, fmt, D, H, knobs, families, shift):
    c = _latest_case(1000 + D + H, fmt, 70, 64, D)
    _check(oracle, mli, dev, request.node.callspec.id, c, "latest", H, knobs, families, shift=shift)


def test_a_dma_shape_takes_the_tiled_kernel(oracle, mli, dev):
    """emb_dim 1536 on bf16 pages is the LDS-DMA kernel's without a table; with one it is a tiled form (64-row tiles at 70 rows)"""
    c = _latest_case(1601, "bf16", 70, 64, 1536, small=True)
    _check(oracle, mli, dev, "bf16-dma-shape-D1536-H12", c, "latest", 12, {}, ("gemm_bf16_rows64", "latest_compact"))


# ---- the fills -----------------------------------------------------------------------------------------------------------------------
def _fill_cases():
    out = []
    for fmt in ("f32", "bf16", "fp8"):
        for fc in (0, 1):
            form = "fill_flat" if fc else "fill_per_row"
            gemm = "gemm_f32_rows64" if fmt == "f32" else "gemm_bf16_fill"
            out.append((f"{fmt}-fill-fc{fc}-H4", fmt, "fill", 128, 4, {"fc": fc, "split": 0}, (gemm, form)))
            for pf in (0, 2):
                fused = "prefill_fused" if pf == 2 or fmt == "fp8" else "prefill_two_launch"
                out.append((f"{fmt}-prefill-fc{fc}-pf{pf}-H2", fmt, "prefill", 128, 2, {"fc": fc, "pf": pf, "split": 0}, (gemm, form, fused)))
    out.append(("f32-fill-split-D256-H4", "f32", "fill", 256, 4, {"fc": 1, "split": 1}, ("gemm_f32_rows64_split", "fill_flat")))
    out.append(("f32-fill-scalar-loads-D68-H1", "f32", "fill", 68, 1, {"fc": 1}, ("gemm_f32_rows64", "fill_flat")))
    out.append(("bf16-fill-widened-fc1-H4", "bf16", "fill", 128, 4, {"fc": 1, "native": 0}, ("gemm_bf16_widened", "fill_flat")))
    out.append(("bf16-fill-widened-fc0-H4", "bf16", "fill", 128, 4, {"fc": 0, "native": 0}, ("gemm_bf16_widened", "fill_per_row")))
    return out


@pytest.mark.parametrize("fmt,mode,D,H,knobs,families", [pytest.param(*c[1:], id=c[0]) for c in _fill_cases()])
def test_fill(oracle, mli, dev, request, fmt, mode, D, H, knobs, families):
    c, mode = gm.fill_case(2000 + D + H, fmt, "signed", 8, 128, D, mode=mode)
    _check(oracle, mli, dev, request.node.callspec.id, c, mode, H, knobs, families, shift="scalar-loads" in request.node.callspec.id)


@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("fc,pf", [(1, 2), (0, 2), (1, 0), (0, 0)])
def test_live_fill_under_a_window(oracle, mli, dev, fmt, fc, pf):
    """W 32, K 4, rows of 100 tokens: pages 1 .. 3 are dead -- their table entries name a spare page that keeps its bytes, as
    the dead pages do -- and the live tokens rotate by their slot, not their live index."""
    W, K = 32, 4
    rng = np.random.default_rng(3000)
    L = np.array([100, 20, 0, 100, 50, 7, 128, 100], np.int32)
    c = gm.Case(3000, "paged", fmt, "signed", 8, 128, 128, 128, L, rng.permutation(8).astype(np.int32), 8, vocab=40)
    gemm = "gemm_f32_rows64" if fmt == "f32" else "gemm_bf16_fill"
    fused = "prefill_fused" if pf == 2 or fmt == "fp8" else "prefill_two_launch"
    _check(oracle, mli, dev, f"{fmt}-live-fill-fc{fc}-pf{pf}", c, "prefill", 4, {"fc": fc, "pf": pf, "split": 0},
           (gemm, "fill_flat" if fc else "fill_per_row", fused), W=W, K=K)


LIVE_FILL_FORMS = [
    # The other kernels of the live fill (tests/kernel_coverage.json): gemm_f32_mfma_rope_kernel<kPagedFillLive, ...> and, from the
    # un-rotated call of (b), gemm_f32_mfma_kernel<kPagedFillLive, ...> with the same arguments.
    # id, fmt, D, H, knobs, families, shifted weights
    ("f32-live-fill-split-D256-H4", "f32", 256, 4, {"fc": 1, "pf": 0, "split": 1},           # <5, false, true, false, 1, true>
     ("gemm_f32_rows64_split", "fill_flat", "prefill_two_launch"), False),
    ("f32-live-fill-scalar-loads-D68-H1", "f32", 68, 1, {"fc": 1, "pf": 0, "split": 0},      # <5, false, false, false, 1, false>
     ("gemm_f32_rows64", "fill_flat", "prefill_two_launch"), True),
    ("bf16-live-fill-widened-D128-H4", "bf16", 128, 4, {"fc": 1, "pf": 0, "native": 0},      # <5, false, true, true, 1, false>
     ("gemm_bf16_widened", "fill_flat", "prefill_two_launch"), False),
]


@pytest.mark.parametrize("fmt,D,H,knobs,families,shift", [pytest.param(*c[1:], id=c[0]) for c in LIVE_FILL_FORMS])
def test_live_fill_under_a_window_other_forms(oracle, mli, dev, request, fmt, D, H, knobs, families, shift):
    """test_live_fill_under_a_window's rows and window at the widths and knobs that take the live fill to its split, scalar-load
    and fp32-widened kernels"""
    W, K = 32, 4
    rng = np.random.default_rng(3100 + D)
    L = np.array([100, 20, 0, 100, 50, 7, 128, 100], np.int32)
    c = gm.Case(3100 + D, "paged", fmt, "signed", 8, 128, D, D, L, rng.permutation(8).astype(np.int32), 8, vocab=40)
    _check(oracle, mli, dev, request.node.callspec.id, c, "prefill", H, knobs, families, W=W, K=K, shift=shift)


# ---- positions past slot 127 and the smallest head sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["f32", "bf16", "fp8"])
def test_long_prefill_then_latest(oracle, mli, dev, fmt):
    """n_sequence 4096, emb_dim 128, 4 heads, the table of mli_rope_table(4096, 32, 10000): new rows of 4095, 2049 and 17 tokens
    through mli_fill_new_k_v_cache_paged_rope (fp8 pages: the lean composition, one head of 128), then
    mli_get_latest_k_q_v_paged_rope at those lengths -- slots 4094, 2048 and 16.  Every K row the fill writes (slots 0, 127, 128,
    2048 and 4094 among them, not a sample) and q are judged; V, x and slot 0 keep the bytes of the un-rotated call.
    "gemm_f32_rope" / "gemm_bf16_rope" counts the launch."""
    c, mode = gm.fill_case(4000, fmt, "signed", 3, 4096, 128, mode="fill", lengths=[4095, 2049, 17])
    _check(oracle, mli, dev, f"{fmt}-fill-S4096-H4", c, mode, 4, {}, (), library_table=True)
    _check(oracle, mli, dev, f"{fmt}-latest-S4096-H4", c, "latest", 4, {"lc": 0}, (), library_table=True)


SMALL_HEADS = [(fmt, H) for fmt in ("f32", "bf16", "fp8") for H in (32, 16, 8)]


@pytest.mark.parametrize("fmt,H", SMALL_HEADS)
def test_smallest_head_sizes(oracle, mli, dev, fmt, H):
    """emb_dim 64 with 32, 16 and 8 heads -- head sizes 2 (one pair per head: rope_half 1), 4 and 8, the near side of the rule
    in rope_half -- at n_sequence 64: the decode projection and the prefill.  The epilogue pairs columns with a quad permute
    whatever the head size; the frequency index is what changes.  The rope counter counts each launch."""
    _check(oracle, mli, dev, f"{fmt}-latest-D64-H{H}", _latest_case(5000 + H, fmt, 70, 64, 64), "latest", H, {"lc": 0}, ())
    c, mode = gm.fill_case(5100 + H, fmt, "signed", 8, 64, 64, mode="prefill")
    _check(oracle, mli, dev, f"{fmt}-prefill-D64-H{H}", c, mode, H, {}, ())
