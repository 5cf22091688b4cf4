"""Early page release through the engine C ABI (mli_engine_set_page_release, mli_engine_get_page_stats): n_batch 8,
n_sequence 256, emb_dim 128, n_vocab 1024, window 40 with 4 sinks; 16 items with prompts of 3 .. 20 tokens and two prompts of
100 and 200 tokens, which are admitted (and, after a preemption, re-admitted) with a gap between their sink page and their
window already.

Release changes which pages a row holds and what its prefill covers, never what a scan reads, and the kernels are
deterministic: every release-on run must produce exactly the tokens of the release-off engine of the same kind on the
worst-case pool (bf16 with mli_tune("bf16_native_mfma", 0), as the window tests run it) -- in both loops, with several rounds
per forward, step graphs, sampled items, and in pools down to 8 pages, where the engine without release cannot hold one row.
Every release-on run is also audited token by token against the float64 replay (tests/replay_model.py).

The sampled items draw with temperature 0.8, top_p 0.95 and seed SAMPLE_SEED + id.  test_sampled_items audits the release-off
reference too: a draw that the reference engine itself makes differently from the replay (seeds 4000 + id: PAGED_BF16, one
head, item 14 at position 28, 6.7e-4 of cumulative mass from the top-p boundary) is then seen to be no effect of release."""
import functools

import pytest

import replay_model as rm
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, W, K = 8, 256, 128, 1024, 40, 4
SEED = 7051
WORST_CASE_BLOCKS = B * S // 16
KINDS = [("PAGED", 1), ("PAGED", 4), ("PAGED_GEMM", 1), ("PAGED_GEMM", 4), ("PAGED_BF16", 1), ("PAGED_BF16", 4), ("PAGED_FP8", 1)]


def _bound(ahead, window=W, sinks=K):
    """pages a row holds at most: ceil(K / 16) + ceil((W + look-ahead) / 16) + 1"""
    return -(-sinks // 16) + -(-(window + ahead) // 16) + 1


@functools.lru_cache(maxsize=1)
def _setup():
    items = make_items(SEED + 1000, 16, 3, 20)
    long_ones = make_items(SEED + 2000, 2, 100, 100)
    items.append((16, long_ones[0][1]))
    items.append((17, make_items(SEED + 3000, 1, 200, 200)[0][1]))
    # the two long prompts are admitted with a gap between the sink page and the window's first page already
    assert [len(t) for _, t in items[16:]] == [100, 200] and all(3 <= len(t) <= 20 for _, t in items[:16])
    assert (100 - W) // 16 > -(-K // 16) and K + W + 32 < S
    return make_model(SEED, V, S, D), items


def _engine(kind_name, **kw):
    from min_llm_inference_amd import engine as eng
    model, _ = _setup()
    kw.setdefault("n_blocks", WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


SAMPLE_SEED = 5000


def _sampling(item_id):
    return dict(temperature=0.8, top_p=0.95, seed=SAMPLE_SEED + item_id)


def _run(kind_name, n_heads=1, release=True, window=W, sinks=K, n_blocks=WORST_CASE_BLOCKS, rounds=1, pipelined=False,
         graphs=False, sampled=False, release_first=False, audit=None):
    """One engine run; returns ({id: tokens}, page stats).  A release-on run (and a release-off one on request) is audited
    against the float64 replay."""
    model, items = _setup()
    if release_first:       # set_page_release before the window and the sinks exist
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=n_heads, release_pages=release)
        if window is not None:
            e.set_window(window)
        if sinks is not None:
            e.set_sinks(sinks)
    else:
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=n_heads, window=window, sinks=sinks,
                    release_pages=release)
    if graphs:
        e.use_private_stream()
        e.configure(step_graphs=True)
    e.set_pipelined(pipelined)
    for item_id, toks in items:
        e.add_item(item_id, toks, **(_sampling(item_id) if sampled else {}))
    try:
        st = e.run()
        finished = e.finished()
        pages = e.page_stats()
    finally:
        e.close()
    assert st.finished == len(items)
    assert pages.pool_pages == n_blocks and pages.in_use == 0 and pages.peak_in_use <= n_blocks
    if release if audit is None else audit:
        store = {"PAGED_BF16": "bf16", "PAGED_FP8": "fp8"}.get(kind_name, "f32")
        spec = rm.Spec(store, n_heads, window, (sinks or 0) if window is not None else 0, flips=store == "fp8")
        sampling = {i: (0.8, 0, 0.95, SAMPLE_SEED + i) for i, _ in items} if sampled else None
        rm.audit(model, items, finished, spec, S, total_tokens=st.total_tokens, sampling=sampling,
                 what=f"page release {kind_name} H{n_heads}, {rounds} round(s), {n_blocks} pages, pipelined {pipelined}").assert_ok()
    if not release:
        assert pages.released_early == 0
    return dict(finished), pages


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (got[k] == want[k]).all(), (what, k)


@pytest.mark.parametrize("kind_name,n_heads", KINDS)
def test_release_never_changes_a_token(mli, dev, kind_name, n_heads):
    from min_llm_inference_amd import MliError
    what = f"{kind_name}, {n_heads} head(s)"
    try:
        assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        ref, ref_pages = _run(kind_name, n_heads, release=False)
        assert ref_pages.preemptions == 0

        def on(text, **kw):
            got, pages = _run(kind_name, n_heads, **kw)
            _same(got, ref, f"{what}: {text}")
            assert pages.released_early > 0, text
            return pages

        on("release on, worst-case pool, sequential loop")
        on("pipelined loop", pipelined=True)
        on("n_forward_rounds 3", rounds=3)
        on("n_forward_rounds 3, pipelined", rounds=3, pipelined=True)
        on("step graphs on a private stream", graphs=True)
        on("set_page_release before set_window / set_sinks", release_first=True)
        # a pool of B rows at the per-row bound (pipelined look-ahead 2 R): nothing is ever preempted
        pool = B * _bound(2)
        pages = on(f"{pool} pages = n_batch x the per-row bound", n_blocks=pool, pipelined=True)
        assert pages.preemptions == 0 and pages.peak_in_use <= pool
        off, off_pages = _run(kind_name, n_heads, release=False, n_blocks=pool, pipelined=True)
        _same(off, ref, f"{what}: release off in {pool} pages")
        assert off_pages.preemptions > 0
        # the bound and two pages: constant preemption, long rows re-prefilled with a gap
        pages = on("per-row bound + 2 pages", n_blocks=_bound(1) + 2)
        assert pages.preemptions > 0
        pages = on("per-row bound + 2 pages, pipelined", n_blocks=_bound(2) + 2, pipelined=True)
        assert pages.preemptions > 0
        # 8 pages < n_sequence / 16: without release no row can reach n_sequence (and the 200-token prompt never starts)
        with pytest.raises(MliError) as err:
            _run(kind_name, n_heads, release=False, n_blocks=8)
        assert "too small" in str(err.value)
        on("8 pages", n_blocks=8)
        on("8 pages, pipelined", n_blocks=8, pipelined=True)
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name,n_heads", KINDS)
def test_sampled_items(mli, dev, kind_name, n_heads):
    try:
        assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        ref, _ = _run(kind_name, n_heads, release=False, sampled=True, audit=True)
        greedy, _ = _run(kind_name, n_heads, release=False)
        assert any(len(ref[k]) != len(greedy[k]) or (ref[k] != greedy[k]).any() for k in ref), "temperature 0.8 decodes greedily"
        for kw in (dict(), dict(pipelined=True), dict(n_blocks=_bound(1) + 2), dict(rounds=3, pipelined=True, n_blocks=B * _bound(6))):
            got, pages = _run(kind_name, n_heads, sampled=True, **kw)
            _same(got, ref, f"{kind_name} sampled, {kw}")
            assert pages.released_early > 0
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


def test_window_without_sinks(mli, dev):
    try:
        assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        ref, _ = _run("PAGED_BF16", 1, release=False, sinks=None)
        with_sinks, _ = _run("PAGED_BF16", 1, release=False)
        assert any(len(ref[k]) != len(with_sinks[k]) or (ref[k] != with_sinks[k]).any() for k in ref)
        for kw in (dict(), dict(pipelined=True, n_blocks=B * _bound(2, W, 0)), dict(n_blocks=_bound(1, W, 0) + 2)):
            got, pages = _run("PAGED_BF16", 1, sinks=None, **kw)
            _same(got, ref, f"(W, K) = (40, 0), {kw}")
            assert pages.released_early > 0
        got, pages = _run("PAGED_BF16", 1, sinks=0, n_blocks=B * _bound(2, W, 0), pipelined=True)
        _same(got, ref, "n_sink = 0")
        assert pages.preemptions == 0
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


def test_without_an_effective_window_release_changes_nothing(mli, dev):
    key = lambda p: (p.pool_pages, p.in_use, p.peak_in_use, p.released_early, p.preemptions)
    for window, sinks in ((None, None), (None, K), (S, K), (W, S - W), (300, 0)):
        plain, plain_pages = _run("PAGED", 1, release=False, window=window, sinks=sinks, n_blocks=WORST_CASE_BLOCKS // 2)
        got, pages = _run("PAGED", 1, release=True, window=window, sinks=sinks, n_blocks=WORST_CASE_BLOCKS // 2)
        _same(got, plain, f"window {window}, sinks {sinks}")
        assert key(pages) == key(plain_pages) and pages.released_early == 0 and pages.preemptions > 0


def test_refusals_and_stats(mli, dev):
    from min_llm_inference_amd import MliError
    _, items = _setup()

    def refused(fn, needle):
        with pytest.raises(MliError) as err:
            fn()
        assert needle in str(err.value), str(err.value)

    e = _engine("CONTIGUOUS", n_blocks=0)
    refused(lambda: e.set_page_release(True), "paged engines")
    refused(lambda: e.set_page_release(False), "paged engines")
    refused(e.page_stats, "no page pool")
    e.close()
    for kind in ("PAGED", "PAGED_GEMM", "PAGED_BF16", "PAGED_FP8"):
        e = _engine(kind, reference_length_reset_quirk=True)
        refused(lambda: e.set_page_release(True), "quirk")
        assert e.page_stats().pool_pages == WORST_CASE_BLOCKS
        e.close()
        e = _engine(kind)
        e.set_page_release(True)              # without a window: accepted
        e.set_page_release(False)
        e.set_window(W)
        e.set_page_release(True)
        e.set_sinks(K)
        e.add_item(*items[17])
        p = e.page_stats()
        assert (p.in_use, p.peak_in_use, p.released_early, p.preemptions) == (0, 0, 0, 0)
        e.step()
        refused(lambda: e.set_page_release(False), "started")
        p = e.page_stats()
        # 200 tokens: the sink page and pages 10 .. 12 of the window and the next position
        assert (p.in_use, p.peak_in_use, p.released_early) == (4, 4, 0), (p.in_use, p.peak_in_use, p.released_early)
        e.close()
