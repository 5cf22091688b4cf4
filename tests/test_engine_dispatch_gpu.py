"""The engines, audited under the kernels their benchmark shapes dispatch ("Engine replay audit").

tests/test_engine_replay_gpu.py audits every token of engines with at most 64 rows and emb_dim 512, where the library's own
dispatch picks the small-shape kernels: the panel fp32 GEMM, the uncompacted projection, the 64-row bf16 tiles, the chunked
scan in grid order.  Here every leg pushes an engine through ONE other branch -- with mli_tune at the smallest shape that
reaches it, or at the benchmark's own shape -- and

  * reads the launch counters (mli_launch_count, per thread, host side) to show that the branch ran, and that it did NOT run
    at the same shape under default knobs (the leg is not vacuous and the knob is what moved it);
  * audits every token with replay_model.audit: no tolerance of its own, every judgement is the audit's (8 x the float32
    forward's own error per item, plus the modelled flip envelope on native bf16 and fp8);
  * where the project documents two paths as bit-identical (panel against tiled GEMM, scan_row_order, nt_loads,
    scan_resident_mib, prefill_fused, fill_compact), also holds the tokens equal to the default run's, item by item.

What an engine adds to the kernels' stand-alone tests: lengths that change every step, admission and preemption punching empty
rows into the batch, new_batch_idx lists, two streams in the pipelined loop, and scratch (arrival counters, the ticket of the
equal-shares scan) allocated once and reused for thousands of launches.

A fill GEMM shares its kernel family with the projection and the logits (fp32: 64-row tiles, wave-split from K 256), so the
fp32 legs count a family's launches NET of the fills ("fill_flat" + "fill_per_row").  The panel kernel and the LDS-DMA
projection have no compacted row list: the compaction leg forces the tiled kernel on the fp32 kind ("gemm_panel" 0) -- with
"latest_compact" 2 alone the counter "latest_compact" stays 0 there.

Every run prints its counters; MLI_REPLAY_REPORT=<file> collects the audit figures as JSON (a line per leg)."""
import functools
import time
import types

import numpy as np
import pytest

import replay_model as rm
from engine_sim import make_items, make_model
from test_engine_replay_gpu import _audited, _kind

pytestmark = pytest.mark.gpu

FAMILIES = ("gemm_f32_panel", "gemm_f32_rows64", "gemm_f32_rows64_split", "gemm_f32_rows128", "gemm_bf16_widened",
            "gemm_bf16_rows64", "gemm_bf16_deep", "gemm_bf16_rows128", "gemm_bf16_dma", "gemm_bf16_fill", "latest_compact",
            "fill_flat", "fill_per_row", "prefill_fused", "prefill_two_launch", "scan_equal_shares", "scan_chunked",
            "scan_rows_ordered", "scan_rows_grid_order", "scan_heads_window")

# include/mli_kernels.h, mli_tune: what every knob a leg touches is restored to
DEFAULTS = dict(gemm_panel=1, gemm_split=1, gemm_tall_tiles=1, gemm_bf16_split=1, latest_compact=1, fill_compact=1,
                prefill_fused=1, scan_stream_min_tokens=1 << 21, scan_stream_dynamic_pct=4, scan_stream_granule=64, nt_loads=2,
                scan_resident_mib=192, scan_row_order=1, bf16_native_mfma=1)

TILED = dict(B=72, S=64, D=256, V=1100)      # 72 rows = one ragged 128-row tile, two 64-row tiles; 1100 = a ragged logits tile
BASE = dict(B=16, S=128, D=64, V=1024)
DMA = dict(B=8, S=64, D=1536, V=1024)
SHARES = dict(B=16, S=1024, D=64, V=1024)
SHARES_WIDE = dict(B=8, S=1024, D=512, V=1024)
ROWS = dict(B=520, S=64, D=64, V=1024)       # more than 512 rows: one workgroup per row, longest first
E1 = dict(B=1024, S=128, D=2048, V=1024)     # bench.py --mode engine


@functools.lru_cache(maxsize=None)
def _workload(name):
    """(model, items): at least twice n_batch items, so every slot is reused (the wide and the LDS-DMA leg: their replay is
    the cost)"""
    if name == "tiled":
        return make_model(9301, TILED["V"], TILED["S"], TILED["D"]), make_items(9302, 2 * TILED["B"] + 6, 1, 40)
    if name == "base":
        return make_model(9311, BASE["V"], BASE["S"], BASE["D"]), make_items(9312, 40, 1, 60)
    if name == "dma":
        return make_model(9321, DMA["V"], DMA["S"], DMA["D"]), make_items(9322, 16, 1, 40)
    if name == "shares":   # rows of very different lengths share a launch, and some reach n_sequence
        return make_model(9331, SHARES["V"], SHARES["S"], SHARES["D"]), make_items(9332, 2 * SHARES["B"], 1, 900)
    if name == "shares wide":
        return make_model(9341, SHARES_WIDE["V"], SHARES_WIDE["S"], SHARES_WIDE["D"]), make_items(9342, 10, 1, 900)
    assert name == "rows"
    return make_model(9351, ROWS["V"], ROWS["S"], ROWS["D"]), make_items(9352, 2 * ROWS["B"], 1, 40)


def _leg(mli, what, variant, wl, shape, knobs=(), **kw):
    """One audited engine run under `knobs` (restored afterwards), with the launch counters of exactly that run."""
    from min_llm_inference_amd import ops
    knobs = dict(knobs)
    knobs.setdefault("bf16_native_mfma", int(_kind(variant)[1]))
    assert set(knobs) <= set(DEFAULTS)
    box = {}

    def after(e):
        box.update(tokens={int(i): t for i, t in e.finished()}, iterations=int(e.stats().iterations),
                   preemptions=int(e.page_stats().preemptions))

    said = ", ".join(f"{k} {v}" for k, v in knobs.items() if v != DEFAULTS[k]) or "default knobs"
    try:
        for k, v in knobs.items():
            assert mli.mli_tune(k.encode(), v) == 0, k
        ops.reset_launch_counts()
        fig = _audited(f"dispatch: {what}; {said}", variant, wl, shape, after=after, **kw)
        counts = {f: ops.launch_count(f) for f in FAMILIES}
    finally:
        for k in knobs:
            mli.mli_tune(k.encode(), DEFAULTS[k])
    print(f"LAUNCHES {variant}, {what}; {said}: iterations {box['iterations']} preemptions {box['preemptions']} "
          + " ".join(f"{f} {n}" for f, n in counts.items() if n))
    fills = counts["fill_flat"] + counts["fill_per_row"]
    return types.SimpleNamespace(fig=fig, counts=counts, fills=fills, **box)


_defaults = {}


def _default(mli, name, variant, shape, **kw):
    """The same shape, kind, loop and pool under default knobs: run once per module, shared, never changed."""
    key = (name, variant, tuple(sorted(kw.items())))
    if key not in _defaults:
        _defaults[key] = _leg(mli, f"{name}, pool of {kw['n_blocks']} pages", variant, _workload(name), shape, **kw)
    return _defaults[key]


def _same_tokens(a, b, what):
    assert a.tokens.keys() == b.tokens.keys(), what
    differ = [i for i in a.tokens if not np.array_equal(a.tokens[i], b.tokens[i])]
    assert not differ, f"{what}: {len(differ)} of {len(a.tokens)} items differ from the default run, first {differ[:5]}"


# ---- fp32: the tiled MFMA kernels instead of the panel kernel -------------------------------------------------------------
@pytest.mark.parametrize("variant", ["PAGED", "PAGED_GEMM"])
def test_tiled_fp32_gemms_instead_of_the_panel_kernel(mli, dev, variant):
    """The projection and the logits on the 64-row tiles with the loader / MFMA wave split (K = 256), on the plain 64-row
    tiles and on the 128-row tiles.  Every tiled kernel is documented bit-identical to the panel kernel: same tokens."""
    wl, kw = _workload("tiled"), dict(n_blocks=3 * TILED["B"], pipelined=True)
    d = _default(mli, "tiled", variant, TILED, **kw)
    c = d.counts
    assert c["gemm_f32_panel"] > 0 and c["gemm_f32_rows128"] == 0 and c["gemm_f32_rows64"] == 0
    assert c["gemm_f32_rows64_split"] == d.fills > 0        # the prefill fill alone is tiled by default

    split = _leg(mli, "tiled", variant, wl, TILED, dict(gemm_panel=0), **kw)
    c = split.counts
    assert c["gemm_f32_panel"] == 0 and c["gemm_f32_rows64"] == 0 and c["gemm_f32_rows128"] == 0
    assert c["gemm_f32_rows64_split"] - split.fills >= split.iterations      # projection and logits of every step
    _same_tokens(split, d, "wave-split 64-row tiles")

    plain = _leg(mli, "tiled", variant, wl, TILED, dict(gemm_panel=0, gemm_split=0), **kw)
    c = plain.counts
    assert c["gemm_f32_panel"] == 0 and c["gemm_f32_rows64_split"] == 0 and c["gemm_f32_rows128"] == 0
    assert c["gemm_f32_rows64"] - plain.fills >= plain.iterations
    _same_tokens(plain, d, "plain 64-row tiles")

    tall = _leg(mli, "tiled", variant, wl, TILED, dict(gemm_panel=0, gemm_split=0, gemm_tall_tiles=2), **kw)
    c = tall.counts
    assert c["gemm_f32_panel"] == 0 and c["gemm_f32_rows64_split"] == 0
    assert c["gemm_f32_rows128"] >= tall.iterations and c["gemm_f32_rows64"] == tall.fills   # the fill keeps 64-row tiles
    _same_tokens(tall, d, "128-row tiles")

    if variant == "PAGED":
        seq = _leg(mli, "tiled, sequential loop", variant, wl, TILED, dict(gemm_panel=0), n_blocks=3 * TILED["B"])
        assert seq.counts["gemm_f32_panel"] == 0 and seq.counts["gemm_f32_rows64_split"] - seq.fills >= seq.iterations
        _same_tokens(seq, d, "wave-split 64-row tiles, sequential loop")


# ---- the decode projection over the compacted list of non-empty rows ------------------------------------------------------
@pytest.mark.parametrize("variant", ["PAGED_GEMM", "PAGED_BF16 exact"])
def test_compacted_projection_with_empty_slots_between_live_rows(mli, dev, variant):
    """latest_compact switches on from emb_dim 1024 by default; here at 256 with a pool of 2 pages per slot, so rows wait for
    a page and finished items leave holes mid-batch.  The fp32 kind is taken off the panel kernel (no row list there)."""
    wl, kw = _workload("tiled"), dict(n_blocks=2 * TILED["B"], pipelined=True)
    off_panel = dict(gemm_panel=0) if variant == "PAGED_GEMM" else {}
    d = _default(mli, "tiled", variant, TILED, **kw)
    assert d.counts["latest_compact"] == 0
    roomy = _default(mli, "tiled", variant, TILED, n_blocks=3 * TILED["B"], pipelined=True)
    assert d.iterations > roomy.iterations      # rows waited for pages: slots stood empty between live rows
    on = _leg(mli, "tiled, 2 pages per slot", variant, wl, TILED, dict(latest_compact=2, **off_panel), **kw)
    assert on.counts["latest_compact"] >= on.iterations
    off = _leg(mli, "tiled, 2 pages per slot", variant, wl, TILED, dict(latest_compact=0, **off_panel), **kw)
    assert off.counts["latest_compact"] == 0
    if variant == "PAGED_GEMM":
        seq = _leg(mli, "tiled, 2 pages per slot, sequential loop", variant, wl, TILED, dict(latest_compact=2, **off_panel),
                   n_blocks=2 * TILED["B"])
        assert seq.counts["latest_compact"] >= seq.iterations


# ---- the prefill's other forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["PAGED_GEMM", "PAGED_BF16 exact"])
def test_uncompacted_fill_and_two_launch_prefill(mli, dev, variant):
    """fill_compact 0: one tile grid per new row; prefill_fused 0: encoder + fill.  Both documented bit-identical."""
    wl, kw = _workload("base"), dict(n_blocks=4 * BASE["B"], pipelined=True)
    d = _default(mli, "base", variant, BASE, **kw)
    assert d.counts["fill_per_row"] == 0 and d.counts["prefill_two_launch"] == 0
    assert d.counts["fill_flat"] > 0 and d.counts["prefill_fused"] > 0
    per_row = _leg(mli, "base", variant, wl, BASE, dict(fill_compact=0), **kw)
    assert per_row.counts["fill_per_row"] > 0 and per_row.counts["fill_flat"] == 0
    _same_tokens(per_row, d, "fill_compact 0")
    two = _leg(mli, "base", variant, wl, BASE, dict(prefill_fused=0), **kw)
    assert two.counts["prefill_two_launch"] > 0 and two.counts["prefill_fused"] == 0
    if variant == "PAGED_BF16 exact":
        assert two.counts["gemm_bf16_fill"] == 0 and d.counts["gemm_bf16_fill"] > 0   # the separate fill is the widened kernel's
    _same_tokens(two, d, "prefill_fused 0")
    if variant == "PAGED_GEMM":
        seq = _leg(mli, "base, sequential loop", variant, wl, BASE, dict(fill_compact=0, prefill_fused=0), n_blocks=4 * BASE["B"])
        assert seq.counts["fill_per_row"] > 0 and seq.counts["prefill_two_launch"] > 0
        _same_tokens(seq, d, "fill_compact 0, prefill_fused 0, sequential loop")


# ---- bf16 / fp8: the 128-row tiles and the LDS-DMA projection -------------------------------------------------------------
@pytest.mark.parametrize("variant", ["PAGED_BF16", "PAGED_FP8"])
def test_tall_bf16_and_fp8_tiles(mli, dev, variant):
    wl, kw = _workload("tiled"), dict(n_blocks=3 * TILED["B"], pipelined=True)
    d = _default(mli, "tiled", variant, TILED, **kw)
    assert d.counts["gemm_bf16_rows128"] == 0 and d.counts["gemm_bf16_deep"] >= d.iterations
    tall = _leg(mli, "tiled", variant, wl, TILED, dict(gemm_tall_tiles=2), **kw)
    assert tall.counts["gemm_bf16_rows128"] >= tall.iterations and tall.counts["gemm_bf16_deep"] == 0
    if variant == "PAGED_BF16":
        seq = _leg(mli, "tiled, sequential loop", variant, wl, TILED, dict(gemm_tall_tiles=2), n_blocks=3 * TILED["B"])
        assert seq.counts["gemm_bf16_rows128"] >= seq.iterations


def test_lds_dma_projection(mli, dev):
    """The default dispatch takes the LDS-DMA kernel from emb_dim 1536 at any batch; gemm_bf16_split 0 is what takes it away."""
    wl = _workload("dma")
    kw = dict(n_blocks=DMA["B"] * DMA["S"] // 32, pipelined=True)
    dma = _default(mli, "dma", "PAGED_BF16", DMA, **kw)
    assert dma.counts["gemm_bf16_dma"] >= dma.iterations and dma.counts["gemm_bf16_rows64"] == 0
    tiled = _leg(mli, "dma", "PAGED_BF16", wl, DMA, dict(gemm_bf16_split=0), **kw)
    assert tiled.counts["gemm_bf16_dma"] == 0 and tiled.counts["gemm_bf16_rows64"] >= tiled.iterations
    seq = _leg(mli, "dma, sequential loop", "PAGED_BF16", wl, DMA, n_blocks=kw["n_blocks"])
    assert seq.counts["gemm_bf16_dma"] >= seq.iterations


# ---- the equal-shares scan ------------------------------------------------------------------------------------------------
def _shares(split):
    return dict(scan_stream_min_tokens=0, scan_stream_dynamic_pct=split[0], scan_stream_granule=split[1])


def _assert_equal_shares_only(run, graphs=False):
    """every step's scan was the equal-shares kernel: no launch handed back to the chunked scan (launch_stream_decode's
    "not applicable" when the scratch is short).  Under step graphs a launch counts once, at capture."""
    c = run.counts
    assert c["scan_chunked"] == 0 and c["scan_heads_window"] == 0, c
    if graphs:
        assert 0 < c["scan_equal_shares"] <= run.iterations, c
    else:
        assert c["scan_equal_shares"] == run.iterations > 0, c


@pytest.mark.parametrize("split", [(4, 64), (12, 16)], ids=["dyn 4 granule 64", "dyn 12 granule 16"])
@pytest.mark.parametrize("variant", ["PAGED", "PAGED_BF16", "PAGED_FP8"])
def test_equal_shares_scan_with_live_counters_and_ticket(mli, dev, variant, split):
    """Prompts of 1 .. 900 tokens at n_sequence 1024 and half the worst-case pool: rows of very different lengths share a
    launch, some reach n_sequence, and rows are preempted and re-prefilled while the arrival counters and the ticket live in
    scratch that thousands of launches reuse."""
    wl, half = _workload("shares"), SHARES["B"] * SHARES["S"] // 32
    d = _default(mli, "shares", variant, SHARES, n_blocks=half, pipelined=True)
    assert d.counts["scan_equal_shares"] == 0 and d.counts["scan_chunked"] == d.iterations and d.preemptions > 0
    for loop, kw in (("sequential loop", dict()), ("pipelined loop", dict(pipelined=True))):
        run = _leg(mli, f"shares, {loop}", variant, wl, SHARES, _shares(split), n_blocks=half, **kw)
        _assert_equal_shares_only(run)
        assert run.preemptions > 0
    if variant == "PAGED":
        for loop, kw in (("step graphs", dict()), ("step graphs, pipelined", dict(pipelined=True))):
            run = _leg(mli, f"shares, {loop}", variant, wl, SHARES, _shares(split), n_blocks=half, graphs=True, **kw)
            _assert_equal_shares_only(run, graphs=True)


def test_equal_shares_scan_at_the_benchmark_width(mli, dev):
    """emb_dim 512 on bf16 pages: the kernel variant of the headline (rows of two lane loads, four segments).  The exact bf16
    GEMM, so that the audit needs no flip envelope at this width."""
    wl, half = _workload("shares wide"), SHARES_WIDE["B"] * SHARES_WIDE["S"] // 32
    variant = "PAGED_BF16 exact"
    d = _default(mli, "shares wide", variant, SHARES_WIDE, n_blocks=half, pipelined=True)
    assert d.counts["scan_equal_shares"] == 0 and d.counts["scan_chunked"] == d.iterations
    for loop, kw in (("sequential loop", dict()), ("pipelined loop", dict(pipelined=True))):
        run = _leg(mli, f"shares wide, {loop}", variant, wl, SHARES_WIDE, dict(scan_stream_min_tokens=0), n_blocks=half, **kw)
        _assert_equal_shares_only(run)


def test_resident_slice_in_motion(mli, dev):
    """nt_loads 1 with scan_resident_mib 1: a slice of the pages is loaded with the default policy, the rest non-temporal,
    while pages change hands between rows.  Documented identical for every value: same tokens as all-default-policy loads."""
    wl, half = _workload("shares"), SHARES["B"] * SHARES["S"] // 32
    kw = dict(n_blocks=half, pipelined=True)
    plain = _leg(mli, "shares, pipelined loop", "PAGED_BF16", wl, SHARES, _shares((4, 64)), **kw)
    _assert_equal_shares_only(plain)
    for mib in (1, 0):
        run = _leg(mli, "shares, pipelined loop", "PAGED_BF16", wl, SHARES,
                   dict(nt_loads=1, scan_resident_mib=mib, **_shares((4, 64))), **kw)
        _assert_equal_shares_only(run)
        _same_tokens(run, plain, f"nt_loads 1, scan_resident_mib {mib}")


# ---- one workgroup per row, longest first ---------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["PAGED", "PAGED_BF16 exact"])
def test_one_item_per_row_longest_first(mli, dev, variant):
    """More than 512 rows of a short sequence: one workgroup per row, rows handed out longest first, over a batch whose
    lengths change every step.  Both orders: identical tokens.
    The pool holds 2 pages per slot.  At n_sequence 64 a row is admitted with its whole table width (DEFAULT_INIT_NUM_BLOCKS
    = 4 pages), so no row ever grows and none is preempted: the short pool keeps half of the slots EMPTY at any time instead,
    scattered through the batch as items finish -- the rows the ranking must pass over (length 0, page count 0)."""
    wl, kw = _workload("rows"), dict(n_blocks=2 * ROWS["B"], pipelined=True)
    d = _default(mli, "rows", variant, ROWS, **kw)
    c = d.counts
    assert c["scan_rows_ordered"] == c["scan_chunked"] == d.iterations > 0 and c["scan_rows_grid_order"] == 0
    grid = _leg(mli, "rows", variant, wl, ROWS, dict(scan_row_order=0), **kw)
    c = grid.counts
    assert c["scan_rows_grid_order"] == c["scan_chunked"] == grid.iterations > 0 and c["scan_rows_ordered"] == 0
    _same_tokens(grid, d, "scan_row_order 0")
    if variant == "PAGED":
        seq = _leg(mli, "rows, sequential loop", variant, wl, ROWS, n_blocks=2 * ROWS["B"])
        assert seq.counts["scan_rows_ordered"] == seq.iterations > 0
        _same_tokens(seq, d, "sequential loop")


# ---- what bench.py --mode engine times ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e1_workload():
    """bench.py run_engine_mode, rank 0: the same generator, draws and scales"""
    B, S, D, V = E1["B"], E1["S"], E1["D"], E1["V"]
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[rm.EOF] *= 1.0001
    sc = 1 / np.sqrt(D)
    model = {"emb_table": emb, "pos_table": u(S, D), "wk": u(D, D, scale=sc), "wq": u(D, D, scale=sc), "wv": u(D, D, scale=sc)}
    items = [(i, rng.integers(0, rm.EOF, size=int(rng.integers(1, 65))).astype(np.int32)) for i in range(2 * B)]
    return model, items


# items audited token by token: a quarter the shortest prompts, a quarter the longest, half drawn with a fixed seed.  The issue's
# 32 on fp32 pages; on native bf16 the flip envelope (16 re-evaluations per item at emb_dim 2048) made 32 items 6.0 - 6.3 s,
# as long as the slowest config-4 tests of test_full_size_properties_gpu.py (6.0 and 6.1 s on their own, under 4.1 s inside the
# whole suite), so the sample is cut there, not the shape
E1_SAMPLE = {"PAGED_GEMM": 32, "PAGED_BF16": 16}


@pytest.mark.parametrize("variant", ["PAGED_GEMM", "PAGED_BF16"])
def test_full_size_engine_run_of_the_benchmark(mli, dev, variant):
    """e1 as bench.py --mode engine builds it: 1024 slots, n_sequence 128, emb_dim 2048, 2048 items with prompts U[1, 64], 4096
    pages, pipelined loop, default knobs -- the default dispatch is the subject.  The bookkeeping judge over all 2048 items,
    the token audit over a sample (E1_SAMPLE; the float64 replay at emb_dim 2048 is the cost of this test).
    Measured on an MI355X box (the TIME line this test prints): PAGED_GEMM 1.4 s in all -- engine 0.18 s, bookkeeping and the
    replay of 32 items 1.2 s; PAGED_BF16 with 32 items 6.3 s -- engine 0.12 s, the replay with its flip envelope 6.2 s -- and
    with the 16 items it keeps 3.5 s, replay 3.3 s."""
    from min_llm_inference_amd import ops
    from test_engine_replay_gpu import _run
    model, items = _e1_workload()
    kind_name, native = _kind(variant)
    t0 = time.perf_counter()
    ops.reset_launch_counts()
    box = {}
    st, finished = _run(kind_name, model, items, E1, E1["B"] * E1["S"] // 32, pipelined=True,
                        after=lambda e: box.update(preemptions=int(e.page_stats().preemptions)))
    counts = {f: ops.launch_count(f) for f in FAMILIES}
    t1 = time.perf_counter()
    print(f"LAUNCHES {variant}, e1 full size: iterations {st.iterations} preemptions {box['preemptions']} "
          + " ".join(f"{f} {n}" for f, n in counts.items() if n))
    assert st.finished == len(items) and st.waiting == 0 and st.in_flight == 0
    assert counts["scan_rows_ordered"] == counts["scan_chunked"] == st.iterations > 0 and counts["scan_equal_shares"] == 0
    assert counts["gemm_f32_panel"] == 0
    if variant == "PAGED_GEMM":
        assert counts["gemm_f32_rows128"] == st.iterations            # the projection of every step, on 128-row tiles
        assert counts["latest_compact"] == st.iterations              # ... over the compacted row list (default from 1024)
        assert counts["gemm_f32_rows64_split"] - (counts["fill_flat"] + counts["fill_per_row"]) == st.iterations   # logits
        assert counts["prefill_two_launch"] > 0 and counts["prefill_fused"] == 0
    else:
        assert counts["gemm_bf16_dma"] == st.iterations and counts["gemm_bf16_rows128"] == 0 and counts["gemm_bf16_rows64"] == 0
    assert box["preemptions"] > 0
    bad = rm.bookkeeping(items, finished, E1["S"], E1["V"], total_tokens=st.total_tokens)
    assert not bad, bad[:5]
    by_len = sorted(range(len(items)), key=lambda i: (len(items[i][1]), i))
    n_sample = E1_SAMPLE[variant]
    q = n_sample // 4
    rest = by_len[q:-q]
    drawn = np.random.default_rng(9361).choice(len(rest), n_sample - 2 * q, replace=False)
    sample = set(by_len[:q] + by_len[-q:] + [rest[i] for i in drawn])
    assert len(sample) == n_sample
    spec = rm.spec_of_kind(kind_name, native=native)
    fig = rm.audit(model, [it for it in items if it[0] in sample], [f for f in finished if int(f[0]) in sample], spec, E1["S"],
                   total_tokens=None, what=f"dispatch: {variant}, e1 full size, pipelined loop, {n_sample} of {len(items)} items")
    t2 = time.perf_counter()
    print(f"TIME {variant}, e1 full size: engine {t1 - t0:.2f} s, bookkeeping + replay of {n_sample} items {t2 - t1:.2f} s")
    fig.assert_ok()
    assert fig.items == n_sample
