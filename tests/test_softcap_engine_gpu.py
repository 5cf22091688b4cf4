"""Attention logit soft-capping through the engine C ABI (mli_engine_set_softcap), at the sizes of tests/test_alibi_engine_gpu.py:
n_batch 8, n_sequence 64, emb_dim 128, n_vocab 1024, 4 query heads (on 4 and on 2 K/V heads), 16 items with prompts of 3 .. 20
tokens, the same model; the cap is softcap_model.ENGINE_CAP (tests/test_softcap_model_cpu.py holds on the CPU that it changes
the tokens of this model).
  - every token of every item is audited against the float64 replay with the cap in its forward (tests/softcap_model.audit:
    replay_model's rules, on the model with expanded Wk / Wv where the heads are grouped);
  - the tokens do not depend on the loop, n_forward_rounds, step graphs, preemption, page release or the order of the setters,
    and a seeded sampled run is reproducible;
  - RoPE beside the cap: audited by the replay with both, other tokens than with either alone;
  - log-probabilities change no token, and PROMPT log-probabilities -- the combination ALiBi and RoPE refuse -- are held to the
    float64 replay with the cap over the prompt rows, under prompt_model.prompt_bound;
  - the tokens differ from those of the engine without the cap and from those under another cap; cap 0 is that engine;
  - with the switch off the engine decodes what it decoded before the switch existed: the head-aware CPU engine's tokens;
  - the refusals of mli_engine_set_softcap and of the setters that come after it."""
import functools

import numpy as np
import pytest

import gqa_model as gm
import heads_model as hm
import prompt_model as pm
import softcap_model as sc
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, H, W, K = 8, 64, 128, 1024, 4, 12, 4
SEED, N_ITEMS = 8648, 16
WORST_CASE_BLOCKS = B * S // 16
KINDS = ["PAGED", "PAGED_GEMM", "PAGED_BF16"]
CAP, THETA, N_TOP = sc.ENGINE_CAP, 10000.0, 3


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(SEED, V, S, D), make_items(SEED + 1000, N_ITEMS, 3, 20)


def _engine(kind_name, **kw):
    from min_llm_inference_amd import engine as eng
    model, _ = _setup()
    kw.setdefault("n_blocks", 0 if kind_name == "CONTIGUOUS" else WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


def _spec(kind_name, window=None, sinks=None, cap=CAP):
    store = "bf16" if kind_name == "PAGED_BF16" else "f32"
    return sc.SoftcapSpec(store, H, window, (sinks or 0) if window is not None else 0, False, float(cap))


def _run(kind_name, cap=CAP, n_kv_heads=H, window=None, sinks=None, release=False, n_blocks=WORST_CASE_BLOCKS, rounds=1,
         pipelined=False, graphs=False, sampled=False, order=None, audit=True, logprobs=None, rope=None, prompt=False):
    """cap None: the engine without the call.  Returns the finished tokens (and the prompt figures with prompt=True)."""
    model, items = _setup()
    if order is None:
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=H, n_kv_heads=n_kv_heads, window=window,
                    sinks=sinks, release_pages=release, logprobs=logprobs, prompt_logprobs=prompt, rope=rope, softcap=cap)
    else:           # the setters in the order given (the cap wants the heads the engine has: after set_heads)
        e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds)
        for what in order:
            {"heads": lambda: e.set_heads(H), "kv": lambda: e.set_kv_heads(n_kv_heads), "window": lambda: e.set_window(window),
             "sinks": lambda: e.set_sinks(sinks), "release": lambda: e.set_page_release(release),
             "softcap": lambda: e.set_softcap(cap)}[what]()
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
    figures = e.finished_prompt_logprobs() if prompt else None
    e.close()
    assert st.finished == len(items)
    if audit and not sampled and cap:
        expanded = gm.expand_model(model, H, n_kv_heads)
        what = f"softcap engine {kind_name} Hkv {n_kv_heads}, {rounds} round(s), {n_blocks} pages, pipelined {pipelined}, rope {rope}"
        if rope is not None:
            import rope_model as rp
            sc.rope_audit(expanded, items, finished, _spec(kind_name, window, sinks, cap), rp.standard_table(S, D // H, rope), S,
                          total_tokens=st.total_tokens, what=what).assert_ok()
        else:
            sc.audit(expanded, items, finished, _spec(kind_name, window, sinks, cap), S, total_tokens=st.total_tokens,
                     what=what).assert_ok()
    return (out, figures) if prompt else out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (got[k] == want[k]).all(), (what, k)


def _differ(a, b):
    return any(len(a[k]) != len(b[k]) or (a[k] != b[k]).any() for k in a)


@pytest.mark.parametrize("n_kv_heads", [H, 2])
@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_a_cap_is_audited_and_independent_of_scheduling(mli, dev, kind_name, n_kv_heads):
    try:
        if kind_name == "PAGED_BF16":     # K / V bits equal to the CPU's (tests/test_engine_gpu.py): the audit needs no E_flip
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        what = f"{kind_name}, {H} heads on {n_kv_heads} K/V head(s), cap {CAP:g}"
        base = _run(kind_name, n_kv_heads=n_kv_heads)
        _same(_run(kind_name, n_kv_heads=n_kv_heads, pipelined=True), base, f"{what}: pipelined loop")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, rounds=2), base, f"{what}: n_forward_rounds 2")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, rounds=2, pipelined=True), base, f"{what}: n_forward_rounds 2, pipelined")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, graphs=True), base, f"{what}: step graphs on a private stream")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, n_blocks=WORST_CASE_BLOCKS // 2), base, f"{what}: half the pool (preemption)")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, n_blocks=WORST_CASE_BLOCKS // 2, pipelined=True), base,
              f"{what}: half the pool, pipelined")
        _same(_run(kind_name, n_kv_heads=n_kv_heads, logprobs=2), base, f"{what}: with log-probabilities")
        plain = _run(kind_name, cap=None, n_kv_heads=n_kv_heads)
        assert _differ(plain, base), "set_softcap is a no-op"
        _same(_run(kind_name, cap=0.0, n_kv_heads=n_kv_heads), plain, f"{what}: cap 0 is the engine without")
        assert _differ(_run(kind_name, cap=4 * CAP, n_kv_heads=n_kv_heads), base), "the engine ignores the cap it is given"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_a_cap_window_sinks_and_page_release(mli, dev, kind_name):
    try:
        if kind_name == "PAGED_BF16":
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        what = f"{kind_name}, {H} heads on 2 K/V heads, window {W}, {K} sinks, cap {CAP:g}"
        base = _run(kind_name, n_kv_heads=2, window=W, sinks=K)
        _same(_run(kind_name, n_kv_heads=2, window=W, sinks=K, release=True), base, f"{what}: release_pages")
        _same(_run(kind_name, n_kv_heads=2, window=W, sinks=K, release=True, pipelined=True, rounds=2), base,
              f"{what}: release_pages, pipelined, n_forward_rounds 2")
        _same(_run(kind_name, n_kv_heads=2, window=W, sinks=K, release=True, n_blocks=WORST_CASE_BLOCKS // 2, graphs=True), base,
              f"{what}: release_pages, half the pool, step graphs")
        for order in (("heads", "kv", "softcap", "window", "sinks", "release"), ("release", "sinks", "window", "heads", "softcap", "kv"),
                      ("window", "heads", "sinks", "kv", "release", "softcap")):
            _same(_run(kind_name, n_kv_heads=2, window=W, sinks=K, release=True, order=order), base, f"{what}: set_* in the order {order}")
        assert _differ(_run(kind_name, n_kv_heads=2), base), "the window is a no-op beside the cap"
        assert _differ(_run(kind_name, cap=None, n_kv_heads=2, window=W, sinks=K), base), "the cap is a no-op beside the window"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_a_cap_and_rope(mli, dev, kind_name):
    """Gemma 2's pair: the rotation in the GEMM epilogues, the cap in the scan.  Audited by the replay with both."""
    try:
        if kind_name == "PAGED_BF16":
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        both = _run(kind_name, n_kv_heads=2, rope=THETA)
        _same(_run(kind_name, n_kv_heads=2, rope=THETA, pipelined=True, n_blocks=WORST_CASE_BLOCKS // 2), both,
              f"{kind_name} RoPE + cap: half the pool, pipelined")
        assert _differ(both, _run(kind_name, n_kv_heads=2)), "the rotation is dropped beside the cap"
        assert _differ(both, _run(kind_name, cap=None, n_kv_heads=2, rope=THETA)), "the cap is dropped beside the rotation"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name,n_kv_heads,window,sinks", [("PAGED", H, None, None), ("PAGED_GEMM", 2, 40, 4), ("PAGED_BF16", 2, None, None)])
def test_prompt_logprobs_of_an_engine_with_a_cap_are_the_capped_replays(mli, dev, kind_name, n_kv_heads, window, sinks):
    """An engine with a cap scores its prompts under the model it decodes with.  Per item: n_scored == n_prompt - 1, and every
    token log-probability and alternative within prompt_model.prompt_bound of the float64 capped replay over the prompt rows;
    the same figures scored WITHOUT the cap in the replay miss that bound somewhere (the prompt scan does not drop the cap)."""
    import replay_model as rm
    model, items = _setup()
    try:
        if kind_name == "PAGED_BF16":
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
        tokens, figures = _run(kind_name, n_kv_heads=n_kv_heads, window=window, sinks=sinks, logprobs=N_TOP, prompt=True)
        _same(_run(kind_name, n_kv_heads=n_kv_heads, window=window, sinks=sinks, audit=False), tokens, "prompt log-probabilities change a token")
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)
    expanded = gm.expand_model(model, H, n_kv_heads)
    spec = _spec(kind_name, window, sinks)
    uncapped = rm.Spec(spec.store, H, spec.window, spec.n_sink, False)
    assert sorted(figures) == sorted(tokens)
    worst_ratio, plain_ratio = 0.0, 0.0
    for item_id, prompt in items:
        p = len(prompt)
        lp, ids, tops = figures[item_id]
        assert len(lp) == p - 1 and ids.shape == (p - 1, N_TOP) and tops.shape == (p - 1, N_TOP), (item_id, len(lp), p)
        toks = np.asarray(tokens[item_id])
        with sc.capped_forward():
            rep = pm.prompt_replay(expanded, toks, p, spec)
        bound, _ = pm.prompt_bound(rep)
        given = pm.prompt_targets(toks, p - 1)
        for which, lg in (("capped", rep.logits), ("plain", pm.prompt_replay(expanded, toks, p, uncapped).logits)):
            m = lg.max(axis=1, keepdims=True)
            lp64 = lg - m - np.log(np.exp(lg - m).sum(axis=1, keepdims=True))
            e_tok = np.abs(lp.astype(np.float64) - lp64[np.arange(p - 1), given])
            e_top = np.abs(tops.astype(np.float64) - np.take_along_axis(lp64, ids.astype(np.int64), axis=1))
            err = max(float(e_tok.max()), float(e_top.max()))
            if which == "plain":
                plain_ratio = max(plain_ratio, err / bound)
                continue
            assert err <= bound, f"{kind_name}: item {item_id}: a prompt logprob is {err:.3e} from the capped replay's, bound {bound:.3e}"
            worst_ratio = max(worst_ratio, err / bound)
    print(f"SOFTCAP PROMPT LOGPROBS engine {kind_name} Hkv {n_kv_heads} W {window}: worst error {worst_ratio:.3g} of the bound; "
          f"against the replay without the cap {plain_ratio:.3g}")
    assert plain_ratio >= 4.0, "the figures are those of the model without the cap"


@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_without_the_switch_decodes_what_it_decoded_before(mli, dev, kind_name):
    """2 K/V heads, no cap: the head-aware CPU engine's tokens on the expanded model, which the engine decoded before the switch
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
        _same(_run(kind_name, cap=None, n_kv_heads=2), cpu, f"{kind_name} without set_softcap against the CPU engine")
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


def test_sampled_run_with_a_cap_is_reproducible_and_loop_independent(mli, dev):
    a = _run("PAGED_BF16", sampled=True)
    _same(_run("PAGED_BF16", sampled=True), a, "sampled run, again")
    _same(_run("PAGED_BF16", sampled=True, pipelined=True), a, "sampled run, pipelined loop")
    assert _differ(a, _run("PAGED_BF16", audit=False)), "temperature 0.8 decodes greedily"
    assert _differ(a, _run("PAGED_BF16", cap=None, sampled=True)), "the sampled run ignores the cap"


def test_set_softcap_refusals(mli, dev):
    from min_llm_inference_amd import MliError
    _, items = _setup()

    def refused(fn, *needles):
        with pytest.raises(MliError) as err:
            fn()
        for needle in needles:
            assert needle in str(err.value), str(err.value)

    for kind in ("CONTIGUOUS", "PAGED_FP8"):
        e = _engine(kind)
        refused(lambda: e.set_softcap(CAP), "mli_engine_set_softcap", "paged")
        e.close()
    for kind in KINDS:
        e = _engine(kind)
        refused(lambda: e.set_softcap(CAP), "mli_engine_set_softcap", "n_heads")     # one head
        e.set_softcap(0.0)                                                           # nothing to turn off: accepted
        e.set_heads(H)
        for bad in (-1.0, -0.5, float("nan"), float("inf"), -float("inf")):
            refused(lambda: e.set_softcap(bad), "mli_engine_set_softcap", "finite")
        e.set_softcap(CAP)
        e.set_softcap(30.0)                                             # again, with another value: accepted before the start
        e.set_heads(H)                                                  # the same count: nothing to change
        refused(lambda: e.set_heads(1), "mli_engine_set_softcap")       # the cap wants two heads
        refused(lambda: e.set_alibi(), "mli_engine_set_alibi", "mli_engine_set_softcap")
        refused(lambda: e.set_alibi([0.5] * H), "mli_engine_set_softcap")
        e.set_logprobs(2)
        e.set_prompt_logprobs(True)                                     # the combination ALiBi and RoPE refuse
        e.set_kv_heads(2)                                               # every other option composes
        e.set_window(W)
        e.set_sinks(K)
        e.set_softcap(0.0)                                              # off again: ALiBi is free to come
        e.set_prompt_logprobs(False)
        e.set_alibi()
        refused(lambda: e.set_softcap(CAP), "mli_engine_set_softcap", "ALiBi")       # the other order
        e.close()
        e = _engine(kind, n_heads=H, logprobs=0, prompt_logprobs=True)
        e.set_softcap(CAP)                                              # after the prompt switch, too
        e.close()
    # lean layers only: with lean layers off an engine cannot have two heads (set_heads refuses them), so set_softcap on it is
    # refused for its one head; what is left to test is lean_layers = 0 AFTER the cap
    e = _engine("PAGED", n_heads=1)
    e.configure(lean_layers=False)
    refused(lambda: e.set_heads(H), "lean")
    refused(lambda: e.set_softcap(CAP), "mli_engine_set_softcap", "n_heads must be >= 2")
    e.configure(lean_layers=True)
    e.set_heads(H)
    e.set_softcap(CAP)
    refused(lambda: e.configure(lean_layers=False), "mli_engine_set_softcap", "lean")
    # after the first step the cap stays
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_softcap(CAP), "started")
    refused(lambda: e.set_softcap(0.0), "started")
    e.close()
    e = _engine("PAGED_BF16", n_heads=H)
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_softcap(CAP), "started")
    e.close()
    assert mli.mli_engine_set_softcap(None, CAP) == -1 and b"null argument" in mli.mli_engine_last_error()
