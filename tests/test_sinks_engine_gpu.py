"""Attention sinks through the engine C ABI (mli_engine_set_sinks): n_batch 8, n_sequence 64, emb_dim 128, n_vocab 1024,
16 items with prompts of 3 .. 20 tokens, window 12 and 4 sinks -- every item outgrows sinks + window, the window
straddles pages and the hole starts inside the sinks' page.  The fp32 and bf16 paged kinds, with 1 and 4 heads, must decode
every item exactly as the sink-aware CPU engine (tests/sinks_model.py: fill + latest from the oracle, then the three stages
per head on the first 4 and the newest 12 tokens; its bf16 mode for bf16 pages), and the tokens must not depend on the loop,
n_forward_rounds, step graphs or preemption.  The fp8 kind (one head) is compared by the 85 % rule of
tests/test_window_engine_gpu.py: a stored K / V element can land on the other side of a rounding boundary, so at least
85 % of the items are token-identical to the CPU engine on fp8-rounded state, and scheduling never changes an item's tokens.

Exact token equality is only well-posed away from ties, so the CPU engine records the smallest gap between the two largest
logits of the run and the tests assert it exceeds 1e-3 (the engines' logits differ from the CPU's by ~1e-5).  The model
seed was picked on the CPU for that, as in tests/test_window_engine_gpu.py: seeds 7000 .. 7051 of (make_model(seed),
make_items(seed + 1000, 16 items)) were tried in order, 7051 is the first whose four runs (1 and 4 heads, fp32 and bf16) all
stay above 1.2e-3: 1.75e-3 (1 head, fp32), 2.21e-3 (1 head, bf16), 2.47e-3 (4 heads, fp32), 2.17e-3 (4 heads, bf16).  (With
24 items none of the seeds 3557 .. 6800 did.)"""
import functools

import numpy as np
import pytest

import replay_model as rm
import sinks_model as sm
import window_model as wm
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, W, K = 8, 64, 128, 1024, 12, 4
SEED, N_ITEMS = 7051, 16
WORST_CASE_BLOCKS = B * S // 16


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(SEED, V, S, D), make_items(SEED + 1000, N_ITEMS, 3, 20)


@functools.lru_cache(maxsize=4)
def _cpu(n_heads, bf16):
    import oracle
    oracle.lib()
    model, items = _setup()
    tokens, gap = sm.run_sinks_cpu_engine(oracle, model, items, B, S, n_heads, W, K, bf16=bf16)
    print(f"SINKS engine: CPU run heads={n_heads} bf16={bf16}: smallest top-2 logit gap {gap:.3e}")
    assert gap > 1e-3, gap
    return tokens


def _engine(kind_name, **kw):
    from min_llm_inference_amd import engine as eng
    model, _ = _setup()
    kw.setdefault("n_blocks", WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


def _run(kind_name, n_heads=1, window=W, sinks=K, n_blocks=WORST_CASE_BLOCKS, rounds=1, pipelined=False, graphs=False,
         sampled=False, order=None, audit=False):
    model, items = _setup()
    if order is None:
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=n_heads, window=window, sinks=sinks)
    else:           # the three setters in the order given
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds)
        for what in order:
            {"heads": lambda: e.set_heads(n_heads), "window": lambda: e.set_window(window), "sinks": lambda: e.set_sinks(sinks)}[what]()
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
        spec = rm.Spec(store, n_heads, window, (sinks or 0) if window is not None else 0, flips=store == "fp8")
        rm.audit(model, items, finished, spec, S, total_tokens=st.total_tokens,
                 what=f"sinks engine {kind_name}, {rounds} round(s), {n_blocks} pages, pipelined {pipelined}").assert_ok()
    return out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (got[k] == want[k]).all(), (what, k)


def _differ(a, b):
    return any(len(a[k]) != len(b[k]) or (a[k] != b[k]).any() for k in a)


def test_every_item_outgrows_sinks_and_window():
    _, items = _setup()
    assert all(3 <= len(t) <= 20 for _, t in items) and W % 16 != 0 and 0 < K < 16 and K + W + 16 < S


@pytest.mark.parametrize("n_heads", [1, 4])
@pytest.mark.parametrize("kind_name", ["PAGED", "PAGED_GEMM", "PAGED_BF16"])
def test_engine_with_sinks_decodes_what_the_cpu_engine_decodes(mli, dev, kind_name, n_heads):
    bf16 = kind_name == "PAGED_BF16"
    cpu = _cpu(n_heads, bf16)
    try:
        if bf16:     # K / V bits equal to the CPU's (tests/test_engine_gpu.py: the native bf16 MFMA sums in another order)
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        what = f"{kind_name}, {n_heads} head(s)"
        base = _run(kind_name, n_heads, audit=True)
        _same(base, cpu, f"{what}: sequential loop against the CPU engine")
        _same(_run(kind_name, n_heads, pipelined=True, audit=True), base, f"{what}: pipelined loop")
        _same(_run(kind_name, n_heads, rounds=2, audit=True), base, f"{what}: n_forward_rounds 2 (sinks and window follow the device-side length)")
        _same(_run(kind_name, n_heads, graphs=True, audit=True), base, f"{what}: step graphs on a private stream")
        _same(_run(kind_name, n_heads, n_blocks=WORST_CASE_BLOCKS // 2, audit=True), base, f"{what}: half the pool (growth + preemption)")
        for order in (("sinks", "window", "heads"), ("heads", "sinks", "window"), ("window", "heads", "sinks")):
            _same(_run(kind_name, n_heads, order=order, audit=True), base, f"{what}: set_* in the order {order}")
        cut = _run(kind_name, n_heads, sinks=None, audit=True)
        assert _differ(cut, base), "set_sinks is a no-op"
        _same(_run(kind_name, n_heads, sinks=0, audit=True), cut, f"{what}: n_sink = 0 is the window alone")
        whole = _run(kind_name, n_heads, window=None, sinks=None, audit=True)
        _same(_run(kind_name, n_heads, window=None, audit=True), whole, f"{what}: sinks without a window change nothing")
        _same(_run(kind_name, n_heads, sinks=S - W, audit=True), whole, f"{what}: n_sink + window = n_sequence is no window")
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


def test_fp8_engine_with_sinks(oracle, mli, dev):
    model, items = _setup()
    cpu, _ = sm.run_sinks_cpu_engine(oracle, model, items, B, S, 1, W, K, bf16="fp8")
    # audit=True: every item of these runs is judged token by token against the float64 replay (tests/replay_model.py)
    outs = [_run("PAGED_FP8", pipelined=True, n_blocks=WORST_CASE_BLOCKS // 2, audit=True), _run("PAGED_FP8", rounds=2, audit=True)]
    for got in outs:
        same = 0
        for item_id, toks in items:
            assert (got[item_id][:len(toks)] == toks).all()
            assert len(got[item_id]) == S or got[item_id][-1] == 1023
            same += len(got[item_id]) == len(cpu[item_id]) and bool((got[item_id] == cpu[item_id]).all())
        print(f"SINKS fp8 engine: {same} of {len(items)} items token-identical to the CPU engine")
        assert same >= 0.85 * len(items), same
        rm.first_divergences(model, items, got, cpu, rm.Spec("fp8", 1, W, K, flips=True), what="sinks fp8 engine")
    _same(outs[1], outs[0], "fp8: scheduling (rounds, pool size, loop, preemption) never changes an item's tokens")
    assert _differ(_run("PAGED_FP8", sinks=None, audit=True), outs[0]), "set_sinks is a no-op on the fp8 engine"
    _same(_run("PAGED_FP8", order=("sinks", "window")), outs[0], "fp8: set_sinks before set_window")


def test_sampled_run_with_sinks_is_reproducible_and_loop_independent(mli, dev):
    a = _run("PAGED_BF16", 4, sampled=True)
    _same(_run("PAGED_BF16", 4, sampled=True), a, "sampled run, again")
    _same(_run("PAGED_BF16", 4, sampled=True, pipelined=True), a, "sampled run, pipelined loop")
    assert _differ(a, _run("PAGED_BF16", 4)), "temperature 0.8 decodes greedily"
    assert _differ(a, _run("PAGED_BF16", 4, sinks=None, sampled=True)), "the sampled run ignores the sinks"


def test_set_sinks_refusals(mli, dev):
    from min_llm_inference_amd import MliError
    from min_llm_inference_amd import engine as eng
    _, items = _setup()

    def refused(fn, needle):
        with pytest.raises(MliError) as err:
            fn()
        assert needle in str(err.value), str(err.value)

    e = _engine("CONTIGUOUS", n_blocks=0)
    refused(lambda: e.set_sinks(K), "paged engines")
    refused(lambda: e.set_sinks(0), "paged engines")
    refused(lambda: e.set_sinks(-1), "n_sink must be")
    e.close()
    for kind in ("PAGED", "PAGED_GEMM", "PAGED_BF16", "PAGED_FP8"):
        e = _engine(kind)
        refused(lambda: e.set_sinks(-1), "n_sink must be")
        e.set_sinks(K)                                   # without a window: accepted, changes nothing
        e.set_sinks(S + 100)
        e.set_window(W)
        e.set_sinks(K + 1)
        e.set_sinks(0)
        e.close()
    e = _engine("PAGED")
    e.configure(lean_layers=False)
    e.set_sinks(0)                                       # the value it has: nothing to change
    refused(lambda: e.set_sinks(K), "lean")
    e.configure(lean_layers=True)
    e.set_sinks(K)
    e.set_window(W)
    refused(lambda: e.configure(lean_layers=False), "lean")
    # heads, window and sinks in any order: each call validates the combination
    e.set_heads(4)
    refused(lambda: e.set_heads(16), "unsupported")      # head_dim 8
    e.set_sinks(2)
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_sinks(K), "started")
    refused(lambda: e.set_sinks(-1), "n_sink must be")
    e.set_sinks(2)                                       # the value it already has: nothing to change
    e.close()
    # a shape the windowed scan does not take is refused where the window is set, with or without sinks
    model, _ = _setup()
    big = eng.Engine(eng.PAGED, 16400, 32, 64, V, model["emb_table"][:, :64].copy(), model["pos_table"][:32, :64].copy(),
                     model["wk"][:64, :64].copy(), model["wq"][:64, :64].copy(), model["wv"][:64, :64].copy(), n_blocks=8)
    big.set_sinks(K)
    refused(lambda: big.set_window(W), "does not take")
    big.set_window(32)
    big.close()
