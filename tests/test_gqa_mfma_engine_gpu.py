"""The MFMA grouped-query scan through the engine C ABI (mli_engine_set_heads_mfma): one PAGED_BF16 engine at emb_dim 2048 with
16 query heads of 128 on 4 K/V heads, n_batch 4, n_sequence 64, the smallest vocabulary (1024), 10 items with prompts of 3 .. 20
tokens.  mli_engine_set_heads refuses this width, so without the switch the engine cannot be created at all.  The engine gets
the model as it is; every token of every run is audited against the float64 replay (tests/replay_model.audit, under a rotary
table tests/rope_model.audit) on the EXPANDED model (tests/gqa_model.expand_model), on which 16 plain heads are the same
attention.  The runs: with and without a window, with page release, with RoPE, under both loops, and with a pool that must
preempt.  A row is admitted with 4 pages, all a row of 64 tokens ever has, so only an engine that releases pages below its window
(rows hold their live pages only) can run its pool dry at this n_sequence: those runs get 5 pages for 4 rows of up to 2 live
pages.  The refusals are checked in both call orders."""
import functools

import pytest

import gqa_model as gm
import replay_model as rm
import rope_model as rp
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, H, HKV, W = 4, 64, 2048, 1024, 16, 4, 12
SEED, N_ITEMS = 8648, 10
WORST_CASE_BLOCKS = B * S // 16
THETA = 10000.0


@functools.lru_cache(maxsize=1)
def _setup():
    model = make_model(SEED, V, S, D)
    return model, gm.expand_model(model, H, HKV), make_items(SEED + 1000, N_ITEMS, 3, 20)


def _engine(kind_name="PAGED_BF16", **kw):
    from min_llm_inference_amd import engine as eng
    model = _setup()[0]
    kw.setdefault("n_blocks", 0 if kind_name == "CONTIGUOUS" else WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


RUNS = {   # window, release_pages, rope, pipelined, n_blocks
    "plain": (None, False, None, False, WORST_CASE_BLOCKS),
    "plain-pipelined": (None, False, None, True, WORST_CASE_BLOCKS),
    "window-release": (W, True, None, False, WORST_CASE_BLOCKS),
    "window-pipelined": (W, False, None, True, WORST_CASE_BLOCKS),
    "rope": (None, False, THETA, False, WORST_CASE_BLOCKS),
    "rope-window-pipelined": (W, False, THETA, True, WORST_CASE_BLOCKS),
    "preempted": (W, True, None, False, 5),
    "preempted-pipelined": (W, True, None, True, 5),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_engine_on_the_mfma_scan_is_audited(mli, dev, name):
    from min_llm_inference_amd import ops
    window, release, rope, pipelined, n_blocks = RUNS[name]
    _, expanded, items = _setup()
    e = _engine(n_blocks=n_blocks, n_heads=H, n_kv_heads=HKV, heads_mfma=True, window=window, release_pages=release, rope=rope)
    e.set_pipelined(pipelined)
    for item_id, toks in items:
        e.add_item(item_id, toks)
    ops.reset_launch_counts()
    st = e.run()
    finished, pages = e.finished(), e.page_stats()
    e.close()
    assert st.finished == len(items)
    scans = {f: ops.launch_count(f) for f in ops.launch_families() if f.startswith("scan_") and ops.launch_count(f)}
    assert list(scans) == ["scan_gqa_mfma"], scans
    assert (pages.preemptions > 0) == (n_blocks < WORST_CASE_BLOCKS), pages.preemptions
    spec = rm.spec_of_kind("PAGED_BF16", H, window, 0)
    what = dict(total_tokens=st.total_tokens, what=f"gqa mfma engine, {name}")
    if rope is None:
        rm.audit(expanded, items, finished, spec, S, **what).assert_ok()
    else:
        rp.audit(expanded, items, finished, rp.rope_spec(spec, rp.standard_table(S, D // H, rope)), S, **what).assert_ok()


# what the kernel does not have: (the setter, what the refusal names); each is refused after the switch and refuses the switch
EXCLUDED = {
    "sinks": (lambda e: e.set_sinks(4), "sink tokens"),
    "alibi": (lambda e: e.set_alibi(), "ALiBi"),
    "softcap": (lambda e: e.set_softcap(30.0), "soft-capping"),
    "sink_logits": (lambda e: e.set_sink_logits([0.5] * 4), "sink logits"),
    "prompt_logprobs": (lambda e: (e.set_logprobs(0), e.set_prompt_logprobs(True)), "prompt log-probabilities"),
}


def _refused(fn, *needles):
    from min_llm_inference_amd import MliError
    with pytest.raises(MliError) as err:
        fn()
    for needle in needles:
        assert needle in str(err.value), str(err.value)


@pytest.mark.parametrize("name", list(EXCLUDED))
def test_set_heads_mfma_and_what_it_excludes_refuse_each_other_in_both_orders(mli, dev, name):
    from min_llm_inference_amd import engine as eng
    setter, needle = EXCLUDED[name]
    model = make_model(SEED, V, S, 256)     # 4 heads of 64: a width every other setter takes too
    def small():
        return eng.Engine(eng.PAGED_BF16, B, S, 256, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                          model["wv"], n_blocks=WORST_CASE_BLOCKS)
    e = small()
    e.set_heads_mfma(4, 2)
    _refused(lambda: setter(e), "mli_engine_set_heads_mfma", "MFMA")
    e.close()
    e = small()
    e.set_heads(4)
    e.set_window(W)
    setter(e)
    _refused(lambda: e.set_heads_mfma(4, 2), "mli_engine_set_heads_mfma", needle)
    e.close()


def test_set_heads_mfma_refusals(mli, dev):
    items = _setup()[2]
    assert mli.mli_engine_set_heads_mfma(None, H, HKV) == -1 and b"null argument" in mli.mli_engine_last_error()
    for kind in ("CONTIGUOUS", "PAGED", "PAGED_GEMM", "PAGED_FP8"):
        e = _engine(kind)
        _refused(lambda: e.set_heads_mfma(H, HKV), "mli_engine_set_heads_mfma", "bf16 paged engine")
        e.close()
    e = _engine()
    _refused(lambda: e.set_heads(H), "mli_engine_set_heads")            # the width the lane-group scan refuses
    for bad in ((H, 3), (H, 0), (0, 0), (H, 2 * H)):
        _refused(lambda: e.set_heads_mfma(*bad), "divide")
    for bad in ((H, 1), (8, 8), (64, 64)):                               # group 16, head_dim 256, head_dim 32
        _refused(lambda: e.set_heads_mfma(*bad), "unsupported")
    e.configure(lean_layers=False)
    _refused(lambda: e.set_heads_mfma(H, HKV), "lean")
    e.configure(lean_layers=True)
    e.set_heads_mfma(H, H)                                               # plain multi-head attention at a refused width
    e.set_heads_mfma(H, HKV)                                             # again: the counts change
    _refused(lambda: e.configure(lean_layers=False), "mli_engine_set_heads_mfma", "lean")
    _refused(lambda: e.set_heads(8), "mli_engine_set_heads_mfma")
    _refused(lambda: e.set_kv_heads(2), "mli_engine_set_heads_mfma")
    e.set_heads(H)                                                       # the counts it has: nothing to change
    e.set_kv_heads(HKV)
    e.set_rope(THETA)
    _refused(lambda: e.set_heads_mfma(32, 8), "rotary table", "16 heads")
    e.add_item(*items[0])
    e.step()
    _refused(lambda: e.set_heads_mfma(H, HKV), "started")
    e.close()
