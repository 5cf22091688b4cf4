"""Sliding-window attention through the engine C ABI (mli_engine_set_window): n_batch 8, n_sequence 64, emb_dim 128, n_vocab
1024, 24 items with prompts of 3 .. 20 tokens, window 12 -- every item outgrows the window, and the window straddles pages.
The fp32 and bf16 paged kinds, with 1 and 4 heads, must decode every item exactly as the window-aware CPU engine
(tests/window_model.py: fill + latest from the oracle, then the three stages per head on the newest 12 tokens; its bf16 mode
for bf16 pages), and the tokens must not depend on the loop, n_forward_rounds, step graphs or preemption.  The fp8 kind (one
head) is compared the way tests/test_paged_fp8_gpu.py compares its engine: a stored K / V element can land on the other
side of a rounding boundary, so at least 85 % of the items are token-identical to the CPU engine on fp8-rounded state, and
scheduling never changes an item's tokens.

Exact token equality is only well-posed away from ties, so the CPU engine records the smallest gap between the two largest
logits of the run and the tests assert it exceeds 1e-3 (the engines' logits differ from the CPU's by ~1e-5).  The model
seed was picked on the CPU for that: seeds 801 .. 3557 of (make_model(seed), make_items(seed + 1000)) were tried in order,
3557 is the first whose four runs (1 and 4 heads, fp32 and bf16) all stay above 1.2e-3: 1.63e-3 (1 head, fp32), 2.44e-3
(1 head, bf16), 1.80e-3 (4 heads, fp32), 2.36e-3 (4 heads, bf16)."""
import functools

import numpy as np
import pytest

import replay_model as rm
import window_model as wm
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, W = 8, 64, 128, 1024, 12
SEED = 3557
WORST_CASE_BLOCKS = B * S // 16


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(SEED, V, S, D), make_items(SEED + 1000, 24, 3, 20)


@functools.lru_cache(maxsize=4)
def _cpu(n_heads, bf16):
    import oracle
    oracle.lib()
    model, items = _setup()
    tokens, gap = wm.run_window_cpu_engine(oracle, model, items, B, S, n_heads, W, bf16=bf16)
    print(f"WINDOW engine: CPU run heads={n_heads} bf16={bf16}: smallest top-2 logit gap {gap:.3e}")
    assert gap > 1e-3, gap
    return tokens


def _run(kind_name, n_heads=1, window=W, n_blocks=WORST_CASE_BLOCKS, rounds=1, pipelined=False, graphs=False, sampled=False,
         audit=False):
    from min_llm_inference_amd import engine as eng
    model, items = _setup()
    e = eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                   model["wv"], n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=n_heads, window=window)
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
    if audit:
        store = {"PAGED_BF16": "bf16", "PAGED_FP8": "fp8"}.get(kind_name, "f32")
        spec = rm.Spec(store, n_heads, None if window in (None, S) else window, flips=store == "fp8")
        rm.audit(model, items, finished, spec, S, total_tokens=st.total_tokens,
                 what=f"window engine {kind_name}, {rounds} round(s), {n_blocks} pages, pipelined {pipelined}").assert_ok()
    return out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (got[k] == want[k]).all(), (what, k)


def _differ(a, b):
    return any(len(a[k]) != len(b[k]) or (a[k] != b[k]).any() for k in a)


def test_every_item_outgrows_the_window():
    _, items = _setup()
    assert all(3 <= len(t) <= 20 for _, t in items) and W % 16 != 0 and W < 16 < S


@pytest.mark.parametrize("n_heads", [1, 4])
@pytest.mark.parametrize("kind_name", ["PAGED", "PAGED_GEMM", "PAGED_BF16"])
def test_engine_with_a_window_decodes_what_the_cpu_engine_decodes(mli, dev, kind_name, n_heads):
    bf16 = kind_name == "PAGED_BF16"
    cpu = _cpu(n_heads, bf16)
    try:
        if bf16:     # K / V bits equal to the CPU's (tests/test_engine_gpu.py: the native bf16 MFMA sums in another order)
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        what = f"{kind_name}, {n_heads} head(s)"
        base = _run(kind_name, n_heads, audit=True)
        _same(base, cpu, f"{what}: sequential loop against the CPU engine")
        _same(_run(kind_name, n_heads, pipelined=True, audit=True), base, f"{what}: pipelined loop")
        _same(_run(kind_name, n_heads, rounds=3, audit=True), base, f"{what}: n_forward_rounds 3 (the window follows the device-side length)")
        _same(_run(kind_name, n_heads, graphs=True, audit=True), base, f"{what}: step graphs on a private stream")
        _same(_run(kind_name, n_heads, n_blocks=WORST_CASE_BLOCKS // 2, audit=True), base, f"{what}: half the pool (growth + preemption)")
        whole = _run(kind_name, n_heads, window=None, audit=True)
        assert _differ(whole, base), "set_window is a no-op"
        _same(_run(kind_name, n_heads, window=S, audit=True), whole, f"{what}: window = n_sequence is no window")
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


def test_fp8_engine_with_a_window(oracle, mli, dev):
    from engine_sim import run_cpu_engine  # noqa: F401  (the fp8 mode of the CPU engine is CpuEngine's)
    model, items = _setup()
    cpu, _ = wm.run_window_cpu_engine(oracle, model, items, B, S, 1, W, bf16="fp8")
    # audit=True: every item of these runs is judged token by token against the float64 replay (tests/replay_model.py)
    outs = [_run("PAGED_FP8", pipelined=True, n_blocks=WORST_CASE_BLOCKS // 2, audit=True), _run("PAGED_FP8", rounds=2, audit=True)]
    for got in outs:
        same = 0
        for item_id, toks in items:
            assert (got[item_id][:len(toks)] == toks).all()
            assert len(got[item_id]) == S or got[item_id][-1] == 1023
            same += len(got[item_id]) == len(cpu[item_id]) and bool((got[item_id] == cpu[item_id]).all())
        print(f"WINDOW fp8 engine: {same} of {len(items)} items token-identical to the CPU engine")
        assert same >= 0.85 * len(items), same
        rm.first_divergences(model, items, got, cpu, rm.Spec("fp8", 1, W, flips=True), what="window fp8 engine")
    _same(outs[1], outs[0], "fp8: scheduling (rounds, pool size, loop, preemption) never changes an item's tokens")
    assert _differ(_run("PAGED_FP8", window=None, audit=True), outs[0]), "set_window is a no-op on the fp8 engine"


def test_sampled_run_with_a_window_is_reproducible_and_loop_independent(mli, dev):
    a = _run("PAGED_BF16", 4, sampled=True)
    _same(_run("PAGED_BF16", 4, sampled=True), a, "sampled run, again")
    _same(_run("PAGED_BF16", 4, sampled=True, pipelined=True), a, "sampled run, pipelined loop")
    assert _differ(a, _run("PAGED_BF16", 4)), "temperature 0.8 decodes greedily"
    assert _differ(a, _run("PAGED_BF16", 4, window=None, sampled=True)), "the sampled run ignores the window"


def test_set_window_refusals(mli, dev):
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

    e = make(eng.CONTIGUOUS)
    e.set_window(S)                                      # no window is accepted everywhere
    e.set_window(S + 100)
    refused(lambda: e.set_window(W), "paged engines")
    refused(lambda: e.set_window(0), "window")
    e.close()
    for kind in (eng.PAGED, eng.PAGED_GEMM, eng.PAGED_BF16, eng.PAGED_FP8):
        e = make(kind)
        refused(lambda: e.set_window(0), "window must be")
        refused(lambda: e.set_window(-1), "window must be")
        e.set_window(W)
        e.set_window(W + 1)
        e.close()
    e = make(eng.PAGED)
    e.configure(lean_layers=False)
    e.set_window(S)                                      # changes nothing: accepted without the lean compositions too
    refused(lambda: e.set_window(W), "lean")
    e.configure(lean_layers=True)
    e.set_window(W)
    refused(lambda: e.configure(lean_layers=False), "lean")
    # heads and window in either order: each call validates the combination
    e.set_heads(4)
    refused(lambda: e.set_heads(16), "unsupported")      # head_dim 8
    e.set_window(5)
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_window(W), "started")
    e.set_window(5)                                      # the value it already has: nothing to change
    e.close()
    e = make(eng.PAGED, n_heads=4)
    e.set_window(W)
    e.set_heads(2)
    e.close()
    e = make(eng.PAGED)
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_window(W), "started")
    e.set_window(S)
    e.close()
    # a shape the windowed scan does not take: more rows than the arrival counters count
    big = eng.Engine(eng.PAGED, 16400, 32, 64, V, model["emb_table"][:, :64].copy(), model["pos_table"][:32, :64].copy(),
                     model["wk"][:64, :64].copy(), model["wq"][:64, :64].copy(), model["wv"][:64, :64].copy(), n_blocks=8)
    refused(lambda: big.set_window(W), "does not take")
    big.set_window(32)
    big.close()
