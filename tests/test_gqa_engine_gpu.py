"""Grouped-query attention through the engine C ABI (mli_engine_set_kv_heads): n_batch 8, n_sequence 64, emb_dim 128, n_vocab
1024, 4 query heads on 2 K/V heads (and on 1), 16 items with prompts of 3 .. 20 tokens.  The engine gets the model as it is:
Wk / Wv of [D, D], of which only the first n_kv_heads * head_dim output columns matter.  The references see the EXPANDED
model (tests/gqa_model.expand_model: column block h of Wk / Wv is block h // g), on which 4 plain heads are the same
attention:
  - every token of every item is audited against the float64 replay (tests/replay_model.audit) under the multi-head spec;
  - with 2 K/V heads the tokens equal those of the head-aware CPU engine (heads_model / sinks_model) on the expanded model;
and the tokens must not depend on the loop, n_forward_rounds, step graphs, preemption, page release or the order of the setters.

Exact token equality is only well-posed away from ties, so the CPU engine records the smallest gap between the two largest
logits of the run and the tests assert it exceeds 1e-3.  The model seed was picked on the CPU for that, as in
tests/test_sinks_engine_gpu.py: seeds from 8000 on of (make_model(seed), make_items(seed + 1000, 16 items)) were tried in
order; 8648 is the first whose four runs with 2 K/V heads (fp32 and bf16, without a window and with window 12 + 4 sinks) all
stay above 1.2e-3: 1.58e-3, 1.55e-3 (fp32), 1.58e-3, 1.67e-3 (bf16).  With 1 K/V head its fp32 run comes within 2.1e-4 of a tie
(no seed of 8000 .. 9199 keeps all eight runs clear), so that configuration is held to the replay audit, which knows about
ties, and to the independence of scheduling, and not to the CPU engine's tokens."""
import functools

import numpy as np
import pytest

import gqa_model as gm
import heads_model as hm
import replay_model as rm
import sinks_model as sm
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, H, W, K = 8, 64, 128, 1024, 4, 12, 4
SEED, N_ITEMS = 8648, 16
WORST_CASE_BLOCKS = B * S // 16
KINDS = ["PAGED", "PAGED_GEMM", "PAGED_BF16"]


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(SEED, V, S, D), make_items(SEED + 1000, N_ITEMS, 3, 20)


@functools.lru_cache(maxsize=8)
def _cpu(n_kv_heads, bf16, windowed):
    import oracle
    oracle.lib()
    model, items = _setup()
    expanded = gm.expand_model(model, H, n_kv_heads)
    if windowed:
        tokens, gap = sm.run_sinks_cpu_engine(oracle, expanded, items, B, S, H, W, K, bf16=bf16)
    else:
        tokens, gap = hm.run_heads_cpu_engine(oracle, expanded, items, B, S, H, bf16=bf16)
    print(f"GQA engine: CPU run Hkv={n_kv_heads} bf16={bf16} windowed={windowed}: smallest top-2 logit gap {gap:.3e}")
    assert gap > 1e-3, gap
    return tokens


def _engine(kind_name, **kw):
    from min_llm_inference_amd import engine as eng
    model, _ = _setup()
    kw.setdefault("n_blocks", 0 if kind_name == "CONTIGUOUS" else WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


def _run(kind_name, n_kv_heads=2, window=None, sinks=None, release=False, n_blocks=WORST_CASE_BLOCKS, rounds=1, pipelined=False,
         graphs=False, sampled=False, order=None, audit=True):
    model, items = _setup()
    if order is None:
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=H, n_kv_heads=n_kv_heads, window=window,
                    sinks=sinks, release_pages=release)
    else:           # the setters in the order given (the K/V heads divide the heads the engine has: after set_heads)
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds)
        for what in order:
            {"heads": lambda: e.set_heads(H), "kv": lambda: e.set_kv_heads(n_kv_heads), "window": lambda: e.set_window(window),
             "sinks": lambda: e.set_sinks(sinks), "release": lambda: e.set_page_release(release)}[what]()
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
    if audit and not sampled:
        # the multi-head spec on the model with expanded Wk / Wv: what the engine computes on the model it was given
        store = "bf16" if kind_name == "PAGED_BF16" else "f32"
        spec = rm.Spec(store, H, window, (sinks or 0) if window is not None else 0, flips=False)
        rm.audit(gm.expand_model(model, H, n_kv_heads), items, finished, spec, S, total_tokens=st.total_tokens,
                 what=f"gqa engine {kind_name} Hkv {n_kv_heads}, {rounds} round(s), {n_blocks} pages, pipelined {pipelined}").assert_ok()
    return out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (got[k] == want[k]).all(), (what, k)


def _differ(a, b):
    return any(len(a[k]) != len(b[k]) or (a[k] != b[k]).any() for k in a)


@pytest.mark.parametrize("n_kv_heads", [2, 1])
@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_kv_heads_decodes_what_the_cpu_engine_decodes(mli, dev, kind_name, n_kv_heads):
    bf16 = kind_name == "PAGED_BF16"
    cpu = _cpu(n_kv_heads, bf16, False) if n_kv_heads == 2 else None
    try:
        if bf16:     # K / V bits equal to the CPU's (tests/test_engine_gpu.py: the native bf16 MFMA sums in another order)
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        what = f"{kind_name}, {H} heads on {n_kv_heads} K/V head(s)"
        base = _run(kind_name, n_kv_heads)
        if cpu is not None:
            _same(base, cpu, f"{what}: sequential loop against the CPU engine on the expanded model")
        _same(_run(kind_name, n_kv_heads, pipelined=True), base, f"{what}: pipelined loop")
        _same(_run(kind_name, n_kv_heads, rounds=3), base, f"{what}: n_forward_rounds 3")
        _same(_run(kind_name, n_kv_heads, rounds=3, pipelined=True), base, f"{what}: n_forward_rounds 3, pipelined")
        _same(_run(kind_name, n_kv_heads, graphs=True), base, f"{what}: step graphs on a private stream")
        _same(_run(kind_name, n_kv_heads, n_blocks=WORST_CASE_BLOCKS // 2), base, f"{what}: half the pool (growth + preemption)")
        _same(_run(kind_name, n_kv_heads, n_blocks=WORST_CASE_BLOCKS // 2, pipelined=True), base, f"{what}: half the pool, pipelined")
        full = _run(kind_name, H)           # n_kv_heads == n_heads: the multi-head engine on the model as given
        assert _differ(full, base), "set_kv_heads is a no-op"
        _same(_run(kind_name, H, order=("heads",), audit=False), full, f"{what}: n_kv_heads == n_heads changes nothing")
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_kv_heads_window_sinks_and_page_release(mli, dev, kind_name):
    bf16 = kind_name == "PAGED_BF16"
    cpu = _cpu(2, bf16, True)
    try:
        if bf16:
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        what = f"{kind_name}, {H} heads on 2 K/V heads, window {W}, {K} sinks"
        base = _run(kind_name, 2, window=W, sinks=K)
        _same(base, cpu, f"{what}: against the CPU engine on the expanded model")
        _same(_run(kind_name, 2, window=W, sinks=K, release=True), base, f"{what}: release_pages")
        _same(_run(kind_name, 2, window=W, sinks=K, release=True, pipelined=True, rounds=2), base,
              f"{what}: release_pages, pipelined, n_forward_rounds 2")
        _same(_run(kind_name, 2, window=W, sinks=K, release=True, n_blocks=WORST_CASE_BLOCKS // 2, graphs=True), base,
              f"{what}: release_pages, half the pool, step graphs")
        for order in (("heads", "kv", "window", "sinks", "release"), ("release", "sinks", "window", "heads", "kv"),
                      ("window", "heads", "sinks", "kv", "release")):
            _same(_run(kind_name, 2, window=W, sinks=K, release=True, order=order), base, f"{what}: set_* in the order {order}")
        assert _differ(_run(kind_name, 2), base), "the window is a no-op beside K/V heads"
        assert _differ(_run(kind_name, H, window=W, sinks=K), base), "the K/V heads are a no-op beside the window"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


def test_sampled_run_with_kv_heads_is_reproducible_and_loop_independent(mli, dev):
    a = _run("PAGED_BF16", sampled=True)
    _same(_run("PAGED_BF16", sampled=True), a, "sampled run, again")
    _same(_run("PAGED_BF16", sampled=True, pipelined=True), a, "sampled run, pipelined loop")
    assert _differ(a, _run("PAGED_BF16", audit=False)), "temperature 0.8 decodes greedily"
    assert _differ(a, _run("PAGED_BF16", H, sampled=True)), "the sampled run ignores the K/V heads"


def test_set_kv_heads_refusals(mli, dev):
    from min_llm_inference_amd import MliError
    _, items = _setup()

    def refused(fn, *needles):
        with pytest.raises(MliError) as err:
            fn()
        for needle in needles:
            assert needle in str(err.value), str(err.value)

    # fp8 and contiguous kinds have one head: only n_kv_heads == n_heads (= 1) is accepted, and changes nothing
    for kind in ("CONTIGUOUS", "PAGED_FP8"):
        e = _engine(kind)
        e.set_kv_heads(1)
        refused(lambda: e.set_kv_heads(2), "n_kv_heads", "divide")
        refused(lambda: e.set_kv_heads(0), "n_kv_heads")
        e.close()
    for kind in KINDS:
        e = _engine(kind)
        e.set_kv_heads(1)                                    # one head on one K/V head
        refused(lambda: e.set_kv_heads(2), "n_kv_heads", "divide")     # more K/V heads than heads
        e.set_heads(H)
        for bad in (3, 8, 0, -1):
            refused(lambda: e.set_kv_heads(bad), "n_kv_heads")
        e.set_kv_heads(2)
        e.set_kv_heads(H)                                    # back to every head its own K/V head
        e.set_kv_heads(1)
        e.set_heads(2)                                       # 1 divides 2
        e.set_heads(H)
        e.set_kv_heads(2)
        refused(lambda: e.set_heads(1), "n_kv_heads")        # 2 does not divide 1
        e.set_heads(2)                                       # 2 K/V heads on 2 heads: every head its own
        e.set_heads(H)
        e.close()
    # lean layers only, in either order
    e = _engine("PAGED", n_heads=1)
    e.configure(lean_layers=False)
    e.set_kv_heads(1)                                        # nothing to change
    e.configure(lean_layers=True)
    e.set_heads(H)
    e.set_kv_heads(2)
    refused(lambda: e.configure(lean_layers=False), "lean")
    # after the first step the value stays
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_kv_heads(1), "n_kv_heads", "started")
    refused(lambda: e.set_kv_heads(H), "n_kv_heads", "started")
    refused(lambda: e.set_kv_heads(3), "n_kv_heads")
    e.set_kv_heads(2)                                        # the value it already has: nothing to change
    e.close()
    e = _engine("PAGED_BF16", n_heads=H)
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_kv_heads(2), "n_kv_heads", "started")
    e.set_kv_heads(H)
    e.close()
