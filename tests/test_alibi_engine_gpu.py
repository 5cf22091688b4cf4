"""ALiBi through the engine C ABI (mli_engine_set_alibi), at the sizes of tests/test_gqa_engine_gpu.py: n_batch 8, n_sequence 64,
emb_dim 128, n_vocab 1024, 4 query heads (on 4 and on 2 K/V heads), 16 items with prompts of 3 .. 20 tokens, the same model.
  - every token of every item is audited against the float64 replay with the bias in its forward (tests/alibi_model.audit:
    replay_model's rules, on the model with expanded Wk / Wv where the heads are grouped);
  - the tokens do not depend on the loop, n_forward_rounds, step graphs, preemption, page release or the order of the setters,
    and a seeded sampled run is reproducible;
  - the tokens differ from those of the engine without the bias; slopes all zero give that engine's tokens;
  - with the switch off the engine decodes what it decoded before the switch existed: the head-aware CPU engine's tokens, as
    tests/test_gqa_engine_gpu.py holds them (the model seed is the one picked there for its distance from ties);
  - the refusals of mli_engine_set_alibi and of the setters that come after it."""
import functools

import numpy as np
import pytest

import alibi_model as am
import gqa_model as gm
import heads_model as hm
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, H, W, K = 8, 64, 128, 1024, 4, 12, 4
SEED, N_ITEMS = 8648, 16
WORST_CASE_BLOCKS = B * S // 16
KINDS = ["PAGED", "PAGED_GEMM", "PAGED_BF16"]
MIXED = (0.5, -0.0625, 0.0, 0.25)


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(SEED, V, S, D), make_items(SEED + 1000, N_ITEMS, 3, 20)


def _engine(kind_name, **kw):
    from min_llm_inference_amd import engine as eng
    model, _ = _setup()
    kw.setdefault("n_blocks", 0 if kind_name == "CONTIGUOUS" else WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


def _run(kind_name, alibi=True, n_kv_heads=H, window=None, sinks=None, release=False, n_blocks=WORST_CASE_BLOCKS, rounds=1,
         pipelined=False, graphs=False, sampled=False, order=None, audit=True, logprobs=None):
    model, items = _setup()
    if order is None:
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=H, n_kv_heads=n_kv_heads, window=window,
                    sinks=sinks, release_pages=release, logprobs=logprobs, alibi=alibi if alibi is not False else None)
    else:           # the setters in the order given (the slopes count the heads the engine has: after set_heads)
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds)
        for what in order:
            {"heads": lambda: e.set_heads(H), "kv": lambda: e.set_kv_heads(n_kv_heads), "window": lambda: e.set_window(window),
             "sinks": lambda: e.set_sinks(sinks), "release": lambda: e.set_page_release(release),
             "alibi": lambda: e.set_alibi(None if alibi is True else alibi)}[what]()
    if graphs:
        e.use_private_stream()
        e.configure(step_graphs=True)
    e.set_pipelined(pipelined)
    for item_id, toks in items:
        if sampled:
            e.add_item(item_id, toks, temperature=0.8, top_p=0.95, seed=4000 + item_id)
        else:
            e.add_item(item_id, toks)
    st = e.run()
    finished = e.finished()
    out = dict(finished)
    e.close()
    assert st.finished == len(items)
    if audit and not sampled and alibi is not False:
        from min_llm_inference_amd import ops
        slopes = ops.alibi_slopes(H) if alibi is True else np.asarray(alibi, np.float32)
        store = "bf16" if kind_name == "PAGED_BF16" else "f32"
        spec = am.AlibiSpec(store, H, window, (sinks or 0) if window is not None else 0, False, tuple(float(m) for m in slopes))
        am.audit(gm.expand_model(model, H, n_kv_heads), items, finished, spec, S, total_tokens=st.total_tokens,
                 what=f"alibi engine {kind_name} Hkv {n_kv_heads}, {rounds} round(s), {n_blocks} pages, pipelined {pipelined}").assert_ok()
    return out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (got[k] == want[k]).all(), (what, k)


def _differ(a, b):
    return any(len(a[k]) != len(b[k]) or (a[k] != b[k]).any() for k in a)


@pytest.mark.parametrize("n_kv_heads", [H, 2])
@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_alibi_is_audited_and_independent_of_scheduling(mli, dev, kind_name, n_kv_heads):
    try:
        if kind_name == "PAGED_BF16":     # K / V bits equal to the CPU's (tests/test_engine_gpu.py): the audit needs no E_flip
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        what = f"{kind_name}, {H} heads on {n_kv_heads} K/V head(s), standard slopes"
        base = _run(kind_name, n_kv_heads=n_kv_heads)
        _same(_run(kind_name, n_kv_heads=n_kv_heads, pipelined=True), base, f"{what}: pipelined loop")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, rounds=2), base, f"{what}: n_forward_rounds 2")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, rounds=2, pipelined=True), base, f"{what}: n_forward_rounds 2, pipelined")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, graphs=True), base, f"{what}: step graphs on a private stream")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, n_blocks=WORST_CASE_BLOCKS // 2), base, f"{what}: half the pool (preemption)")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, n_blocks=WORST_CASE_BLOCKS // 2, pipelined=True), base,
              f"{what}: half the pool, pipelined")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, logprobs=2), base, f"{what}: with log-probabilities")
        plain = _run(kind_name, alibi=False, n_kv_heads=n_kv_heads)
        assert _differ(plain, base), "set_alibi is a no-op"
        _same(_run(kind_name, alibi=(0.0,) * H, n_kv_heads=n_kv_heads), plain, f"{what}: slopes all zero are the engine without")
        assert _differ(_run(kind_name, alibi=MIXED, n_kv_heads=n_kv_heads), base), "the engine ignores the slopes it is given"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_alibi_window_sinks_and_page_release(mli, dev, kind_name):
    try:
        if kind_name == "PAGED_BF16":
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        what = f"{kind_name}, {H} heads on 2 K/V heads, window {W}, {K} sinks, standard slopes"
        base = _run(kind_name, n_kv_heads=2, window=W, sinks=K)
        _same(_run(kind_name, n_kv_heads=2, window=W, sinks=K, release=True), base, f"{what}: release_pages")
        _same(_run(kind_name, n_kv_heads=2, window=W, sinks=K, release=True, pipelined=True, rounds=2), base,
              f"{what}: release_pages, pipelined, n_forward_rounds 2")
        _same(_run(kind_name, n_kv_heads=2, window=W, sinks=K, release=True, n_blocks=WORST_CASE_BLOCKS // 2, graphs=True), base,
              f"{what}: release_pages, half the pool, step graphs")
        for order in (("heads", "kv", "alibi", "window", "sinks", "release"), ("release", "sinks", "window", "heads", "alibi", "kv"),
                      ("window", "heads", "sinks", "kv", "release", "alibi")):
            _same(_run(kind_name, n_kv_heads=2, window=W, sinks=K, release=True, order=order), base, f"{what}: set_* in the order {order}")
        assert _differ(_run(kind_name, n_kv_heads=2), base), "the window is a no-op beside the slopes"
        assert _differ(_run(kind_name, alibi=False, n_kv_heads=2, window=W, sinks=K), base), "the slopes are a no-op beside the window"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_without_the_switch_decodes_what_it_decoded_before(mli, dev, kind_name):
    """2 K/V heads, no bias: the head-aware CPU engine's tokens on the expanded model, which the engine decoded before ALiBi
    existed (tests/test_gqa_engine_gpu.py; the CPU run's distance from a tie is asserted there and again here)"""
    import oracle
    oracle.lib()
    model, items = _setup()
    bf16 = kind_name == "PAGED_BF16"
    cpu, gap = hm.run_heads_cpu_engine(oracle, gm.expand_model(model, H, 2), items, B, S, H, bf16=bf16)
    assert gap > 1e-3, gap
    try:
        if bf16:
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        _same(_run(kind_name, alibi=False, n_kv_heads=2), cpu, f"{kind_name} without set_alibi against the CPU engine")
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


def test_sampled_run_with_alibi_is_reproducible_and_loop_independent(mli, dev):
    a = _run("PAGED_BF16", sampled=True)
    _same(_run("PAGED_BF16", sampled=True), a, "sampled run, again")
    _same(_run("PAGED_BF16", sampled=True, pipelined=True), a, "sampled run, pipelined loop")
    assert _differ(a, _run("PAGED_BF16", audit=False)), "temperature 0.8 decodes greedily"
    assert _differ(a, _run("PAGED_BF16", alibi=False, sampled=True)), "the sampled run ignores the slopes"


def test_set_alibi_refusals(mli, dev):
    from min_llm_inference_amd import MliError
    _, items = _setup()

    def refused(fn, *needles):
        with pytest.raises(MliError) as err:
            fn()
        for needle in needles:
            assert needle in str(err.value), str(err.value)

    for kind in ("CONTIGUOUS", "PAGED_FP8"):
        e = _engine(kind)
        refused(lambda: e.set_alibi(), "mli_engine_set_alibi", "paged")
        refused(lambda: e.set_alibi([0.5]), "mli_engine_set_alibi")
        e.close()
    for kind in KINDS:
        e = _engine(kind)
        refused(lambda: e.set_alibi(), "n_heads")                       # one head
        refused(lambda: e.set_alibi([0.5]), "n_heads")
        e.set_heads(H)
        for bad in ([0.5] * 3, [0.5] * 5, [0.5] * 8):
            refused(lambda: e.set_alibi(bad), "n_heads")                # n != n_heads
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused(lambda: e.set_alibi([0.5, bad, 0.25, 0.125]), "finite")
        e.set_alibi()
        e.set_alibi([0.5, -0.25, 0.0, 1.0])                             # again, with other values: accepted before the start
        e.set_heads(H)                                                  # the same count: nothing to change
        refused(lambda: e.set_heads(2), "mli_engine_set_alibi")         # the slopes count 4 heads
        e.set_logprobs(2)
        refused(lambda: e.set_prompt_logprobs(True), "ALiBi")
        e.set_kv_heads(2)                                               # every other option composes
        e.set_window(W)
        e.set_sinks(K)
        e.set_page_release(True)
        e.close()
        e = _engine(kind, n_heads=H, logprobs=0, prompt_logprobs=True)
        refused(lambda: e.set_alibi(), "prompt")
        e.close()
    # lean layers only.  Of the two orders one exists: with lean layers off an engine cannot have two heads (set_heads refuses
    # them), so set_alibi on it is refused for its one head -- the setter's own lean-layers check is a second line behind that
    # -- and what is left to test is lean_layers = 0 AFTER the slopes
    e = _engine("PAGED", n_heads=1)
    e.configure(lean_layers=False)
    refused(lambda: e.set_heads(H), "lean")
    refused(lambda: e.set_alibi(), "mli_engine_set_alibi", "n_heads must be >= 2")
    e.configure(lean_layers=True)
    e.set_heads(H)
    e.set_alibi()
    refused(lambda: e.configure(lean_layers=False), "lean")
    # after the first step the slopes stay
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_alibi(), "started")
    refused(lambda: e.set_alibi([0.5] * H), "started")
    e.close()
    e = _engine("PAGED_BF16", n_heads=H)
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_alibi(), "started")
    e.close()
