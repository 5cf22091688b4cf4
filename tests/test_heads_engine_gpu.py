"""Multi-head attention through the engine C ABI (mli_engine_set_heads): n_batch 8, n_sequence 64, emb_dim 128, n_vocab 1024,
4 heads, 24 items with prompts of 3 .. 20 tokens.  The three paged kinds must decode every item exactly as the head-aware CPU
engine (tests/heads_model.py: fill + latest from the oracle, then the three stages per head; its bf16 mode for bf16
pages), and the tokens must not depend on the loop, n_forward_rounds, step graphs or preemption.

Exact token equality is only well-posed away from ties, so the CPU engine records the smallest gap between the two largest
logits of the run and the tests assert it exceeds 1e-3 (the engines' logits differ from the CPU's by ~1e-5).  The model
seed was picked on the CPU for that: seeds 501 .. 758 of (make_model(seed), make_items(seed + 1000)) were tried in order,
758 is the first whose fp32 and bf16 runs both stay above 1.2e-3 (1.35e-3 and 2.9e-3)."""
import functools

import numpy as np
import pytest

import heads_model as hm
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, H = 8, 64, 128, 1024, 4
SEED = 758
WORST_CASE_BLOCKS = B * S // 16


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(SEED, V, S, D), make_items(SEED + 1000, 24, 3, 20)


@functools.lru_cache(maxsize=2)
def _cpu(bf16):
    import oracle
    oracle.lib()
    model, items = _setup()
    tokens, gap = hm.run_heads_cpu_engine(oracle, model, items, B, S, H, bf16=bf16)
    print(f"HEADS engine: CPU run bf16={bf16}: smallest top-2 logit gap {gap:.3e}")
    assert gap > 1e-3, gap
    return tokens


def _run(kind_name, n_heads=H, n_blocks=WORST_CASE_BLOCKS, rounds=1, pipelined=False, graphs=False, sampled=False):
    from min_llm_inference_amd import engine as eng
    model, items = _setup()
    e = eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                   model["wv"], n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=n_heads)
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
    out = dict(e.finished())
    e.close()
    assert st.finished == len(items)
    return out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (got[k] == want[k]).all(), (what, k)


@pytest.mark.parametrize("kind_name", ["PAGED", "PAGED_GEMM", "PAGED_BF16"])
def test_engine_with_heads_decodes_what_the_cpu_engine_decodes(mli, dev, kind_name):
    bf16 = kind_name == "PAGED_BF16"
    cpu = _cpu(bf16)
    try:
        if bf16:     # K / V bits equal to the CPU's (tests/test_engine_gpu.py: the native bf16 MFMA sums in another order)
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        base = _run(kind_name)
        _same(base, cpu, f"{kind_name}: sequential loop against the CPU engine")
        _same(_run(kind_name, pipelined=True), base, f"{kind_name}: pipelined loop")
        _same(_run(kind_name, rounds=3), base, f"{kind_name}: n_forward_rounds 3")
        _same(_run(kind_name, rounds=3, pipelined=True), base, f"{kind_name}: n_forward_rounds 3, pipelined")
        _same(_run(kind_name, graphs=True), base, f"{kind_name}: step graphs on a private stream")
        _same(_run(kind_name, n_blocks=WORST_CASE_BLOCKS // 2), base, f"{kind_name}: half the pool (growth + preemption)")
        _same(_run(kind_name, n_blocks=WORST_CASE_BLOCKS // 2, pipelined=True), base, f"{kind_name}: half the pool, pipelined")
        one = _run(kind_name, n_heads=1)
        assert any(len(one[k]) != len(base[k]) or (one[k] != base[k]).any() for k in base), "set_heads is a no-op"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


def test_sampled_run_with_heads_is_reproducible_and_loop_independent(mli, dev):
    a = _run("PAGED_BF16", sampled=True)
    _same(_run("PAGED_BF16", sampled=True), a, "sampled run, again")
    _same(_run("PAGED_BF16", sampled=True, pipelined=True), a, "sampled run, pipelined loop")
    greedy = _run("PAGED_BF16")
    assert any(len(a[k]) != len(greedy[k]) or (a[k] != greedy[k]).any() for k in a), "temperature 0.8 decodes greedily"


def test_set_heads_refusals(mli, dev):
    from min_llm_inference_amd import MliError
    from min_llm_inference_amd import engine as eng
    model, items = _setup()

    def make(kind, **kw):
        return eng.Engine(kind, B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"], model["wv"],
                          n_blocks=0 if kind == eng.CONTIGUOUS else WORST_CASE_BLOCKS, **kw)

    def refused(fn, needle):
        with pytest.raises(MliError) as err:
            fn()
        assert needle in str(err.value), str(err.value)

    for kind in (eng.CONTIGUOUS, eng.PAGED_FP8):
        e = make(kind)
        e.set_heads(1)                                   # one head is accepted everywhere
        refused(lambda: e.set_heads(H), "paged engines")
        e.close()
    e = make(eng.PAGED)
    refused(lambda: e.set_heads(16), "unsupported")      # head_dim 8
    refused(lambda: e.set_heads(3), "unsupported")       # emb_dim % n_heads
    refused(lambda: e.set_heads(0), "n_heads")
    e.configure(lean_layers=False)
    refused(lambda: e.set_heads(H), "lean")
    e.configure(lean_layers=True)
    e.set_heads(H)
    refused(lambda: e.configure(lean_layers=False), "lean")
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_heads(2), "started")
    e.set_heads(H)                                       # the value it already has: nothing to change
    e.close()
    e = make(eng.PAGED)
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_heads(H), "started")
    e.set_heads(1)
    e.close()
