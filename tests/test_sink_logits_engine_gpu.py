"""Learned attention-sink logits through the engine C ABI (mli_engine_set_sink_logits), at the sizes of
tests/test_softcap_engine_gpu.py: n_batch 8, n_sequence 64, emb_dim 128, n_vocab 1024, 4 query heads on 2 K/V heads, 16 items with
prompts of 3 .. 20 tokens, the same model; the logits are sink_logits_model.ENGINE_LOGITS (tests/test_sink_logits_model_cpu.py
holds on the CPU that they change the tokens of this model).
  - every token of every item is audited against the float64 replay with the sink in its forward (sink_logits_model.audit:
    replay_model's rules, on the model with expanded Wk / Wv), and every prompt figure against that replay over the prompt rows;
  - the tokens do not depend on the loop, n_forward_rounds, step graphs or the pool size (preemption);
  - with a window, sink tokens and page release, and with RoPE (audited by the replay with both);
  - all -inf logits: the tokens, the log-probabilities and the prompt log-probabilities of the engine without the call, bit for bit;
  - the launch counters show that the new families ran and the plain ones did not;
  - the refusals of mli_engine_set_sink_logits and of the setters that come after it, in both orders of every refused pair."""
import functools

import numpy as np
import pytest

import gqa_model as gm
import prompt_model as pm
import sink_logits_model as sl
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, H, HKV, W, K = 8, 64, 128, 1024, 4, 2, 12, 4
SEED, N_ITEMS = 8648, 16
WORST_CASE_BLOCKS = B * S // 16
KINDS = ["PAGED", "PAGED_GEMM", "PAGED_BF16"]
Z, THETA, N_TOP = sl.ENGINE_LOGITS, 10000.0, 3
NONE = tuple(float(t) for t in sl.none(H))


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(SEED, V, S, D), make_items(SEED + 1000, N_ITEMS, 3, 20)


def _engine(kind_name, **kw):
    from min_llm_inference_amd import engine as eng
    model, _ = _setup()
    kw.setdefault("n_blocks", 0 if kind_name == "CONTIGUOUS" else WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


def _spec(kind_name, window=None, sinks=None, z=Z):
    store = "bf16" if kind_name == "PAGED_BF16" else "f32"
    return sl.SinkLogitsSpec(store, H, window, (sinks or 0) if window is not None else 0, False, tuple(float(t) for t in z))


def _run(kind_name, z=Z, window=None, sinks=None, release=False, n_blocks=WORST_CASE_BLOCKS, rounds=1, pipelined=False,
         graphs=False, audit=True, logprobs=None, rope=None, prompt=False, counts=None):
    """z None: the engine without the call.  Returns the finished tokens (with prompt=True: tokens, prompt figures and the
    decoded tokens' log-probabilities)."""
    from min_llm_inference_amd import ops
    model, items = _setup()
    e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=H, n_kv_heads=HKV, window=window, sinks=sinks,
                release_pages=release, logprobs=logprobs, prompt_logprobs=prompt, rope=rope, sink_logits=z)
    if graphs:
        e.use_private_stream()
        e.configure(step_graphs=True)
    e.set_pipelined(pipelined)
    for item_id, toks in items:
        e.add_item(item_id, toks)
    if counts is not None:
        ops.reset_launch_counts()
    st = e.run()
    if counts is not None:
        counts.update({f: ops.launch_count(f) for f in ("scan_heads_sink_logits", "scan_prompt_sink_logits", "scan_heads_window",
                                                        "scan_prompt")})
    finished = e.finished()
    out = dict(finished)
    figures = e.finished_prompt_logprobs() if prompt else None
    chosen = e.finished_logprobs() if prompt and logprobs is not None else None
    e.close()
    assert st.finished == len(items)
    if audit and z is not None and z != NONE:
        expanded = gm.expand_model(model, H, HKV)
        what = f"sink-logit engine {kind_name}, {rounds} round(s), {n_blocks} pages, pipelined {pipelined}, graphs {graphs}, rope {rope}"
        if rope is not None:
            import rope_model as rp
            sl.rope_audit(expanded, items, finished, _spec(kind_name, window, sinks, z), rp.standard_table(S, D // H, rope), S,
                          total_tokens=st.total_tokens, what=what).assert_ok()
        else:
            sl.audit(expanded, items, finished, _spec(kind_name, window, sinks, z), S, total_tokens=st.total_tokens,
                     what=what).assert_ok()
    return (out, figures, chosen) if prompt else out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (np.asarray(got[k]) == np.asarray(want[k])).all(), (what, k)


def _differ(a, b):
    return any(len(a[k]) != len(b[k]) or (a[k] != b[k]).any() for k in a)


def _bf16_exact(mli, kind_name):
    if kind_name == "PAGED_BF16":     # K / V bits equal to the CPU's (tests/test_engine_gpu.py): the audit needs no E_flip
        assert mli.mli_tune(b"bf16_native_mfma", 0) == 0


@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_sink_logits_is_audited_and_independent_of_scheduling(mli, dev, kind_name):
    try:
        _bf16_exact(mli, kind_name)
        what = f"{kind_name}, {H} heads on {HKV} K/V heads, sink logits {Z}"
        counts = {}
        base = _run(kind_name, counts=counts)
        assert counts["scan_heads_sink_logits"] > 0 and counts["scan_heads_window"] == 0 and counts["scan_prompt"] == 0, counts
        _same(_run(kind_name, pipelined=True), base, f"{what}: pipelined loop")
        _same(_run(kind_name, rounds=2), base, f"{what}: n_forward_rounds 2")
        _same(_run(kind_name, rounds=2, pipelined=True), base, f"{what}: n_forward_rounds 2, pipelined")
        _same(_run(kind_name, graphs=True), base, f"{what}: step graphs on a private stream")
        _same(_run(kind_name, n_blocks=WORST_CASE_BLOCKS // 2), base, f"{what}: half the pool (preemption)")
        _same(_run(kind_name, n_blocks=WORST_CASE_BLOCKS // 2, pipelined=True, graphs=True), base,
              f"{what}: half the pool, pipelined, step graphs")
        plain = _run(kind_name, z=None)
        assert _differ(plain, base), "set_sink_logits is a no-op"
        assert _differ(_run(kind_name, z=tuple(-t for t in Z), audit=False), base), "the engine ignores the logits it is given"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name", KINDS)
def test_engine_with_sink_logits_window_sink_tokens_page_release_and_rope(mli, dev, kind_name):
    try:
        _bf16_exact(mli, kind_name)
        what = f"{kind_name}, window {W}, {K} sink tokens, sink logits"
        base = _run(kind_name, window=W, sinks=K)
        _same(_run(kind_name, window=W, sinks=K, release=True), base, f"{what}: release_pages")
        _same(_run(kind_name, window=W, sinks=K, release=True, n_blocks=WORST_CASE_BLOCKS // 2, graphs=True, rounds=2), base,
              f"{what}: release_pages, half the pool, step graphs, n_forward_rounds 2")
        assert _differ(_run(kind_name), base), "the window is a no-op beside the logits"
        assert _differ(_run(kind_name, z=None, window=W, sinks=K), base), "the logits are a no-op beside the window"
        both = _run(kind_name, rope=THETA)
        _same(_run(kind_name, rope=THETA, pipelined=True, n_blocks=WORST_CASE_BLOCKS // 2), both, f"{kind_name} RoPE: half the pool, pipelined")
        assert _differ(both, _run(kind_name, z=None, rope=THETA)), "the logits are dropped beside the rotation"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name,window,sinks", [("PAGED", None, None), ("PAGED_GEMM", 40, 4), ("PAGED_BF16", None, None)])
def test_prompt_logprobs_of_an_engine_with_sink_logits_are_the_replays(mli, dev, kind_name, window, sinks):
    """An engine with sink logits scores its prompts under the model it decodes with.  Per item: n_scored == n_prompt - 1, and
    every token log-probability and alternative within prompt_model.prompt_bound of the float64 replay with the sink over the
    prompt rows; the same figures against the replay WITHOUT the sink miss that bound somewhere."""
    import replay_model as rm
    model, items = _setup()
    try:
        _bf16_exact(mli, kind_name)
        counts = {}
        tokens, figures, _ = _run(kind_name, window=window, sinks=sinks, logprobs=N_TOP, prompt=True, counts=counts)
        assert counts["scan_prompt_sink_logits"] > 0 and counts["scan_prompt"] == 0 and counts["scan_heads_sink_logits"] > 0, counts
        _same(_run(kind_name, window=window, sinks=sinks, audit=False), tokens, "prompt log-probabilities change a token")
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)
    expanded = gm.expand_model(model, H, HKV)
    spec = _spec(kind_name, window, sinks)
    without = rm.Spec(spec.store, H, spec.window, spec.n_sink, False)
    assert sorted(figures) == sorted(tokens)
    worst_ratio, plain_ratio = 0.0, 0.0
    for item_id, prompt in items:
        p = len(prompt)
        lp, ids, tops = figures[item_id]
        assert len(lp) == p - 1 and ids.shape == (p - 1, N_TOP) and tops.shape == (p - 1, N_TOP), (item_id, len(lp), p)
        toks = np.asarray(tokens[item_id])
        with sl.sink_forward():
            rep = pm.prompt_replay(expanded, toks, p, spec)
        bound, _ = pm.prompt_bound(rep)
        given = pm.prompt_targets(toks, p - 1)
        for which, lg in (("sink", rep.logits), ("plain", pm.prompt_replay(expanded, toks, p, without).logits)):
            m = lg.max(axis=1, keepdims=True)
            lp64 = lg - m - np.log(np.exp(lg - m).sum(axis=1, keepdims=True))
            e_tok = np.abs(lp.astype(np.float64) - lp64[np.arange(p - 1), given])
            e_top = np.abs(tops.astype(np.float64) - np.take_along_axis(lp64, ids.astype(np.int64), axis=1))
            err = max(float(e_tok.max()), float(e_top.max()))
            if which == "plain":
                plain_ratio = max(plain_ratio, err / bound)
                continue
            assert err <= bound, f"{kind_name}: item {item_id}: a prompt logprob is {err:.3e} from the replay's, bound {bound:.3e}"
            worst_ratio = max(worst_ratio, err / bound)
    print(f"SINK_LOGITS PROMPT LOGPROBS engine {kind_name} W {window}: worst error {worst_ratio:.3g} of the bound; against the "
          f"replay without the sink {plain_ratio:.3g}")
    assert plain_ratio >= 4.0, "the figures are those of the model without the sink"


@pytest.mark.parametrize("kind_name", KINDS)
def test_all_minus_inf_logits_are_the_engine_without_the_call_bit_for_bit(mli, dev, kind_name):
    counts = {}
    tokens, figures, chosen = _run(kind_name, z=NONE, logprobs=N_TOP, prompt=True, counts=counts)
    assert counts["scan_heads_sink_logits"] > 0 and counts["scan_prompt_sink_logits"] > 0, counts
    assert counts["scan_heads_window"] == 0 and counts["scan_prompt"] == 0, counts
    plain_counts = {}
    want, want_figures, want_chosen = _run(kind_name, z=None, logprobs=N_TOP, prompt=True, counts=plain_counts)
    assert plain_counts["scan_heads_sink_logits"] == 0 and plain_counts["scan_prompt_sink_logits"] == 0, plain_counts
    assert plain_counts["scan_heads_window"] == counts["scan_heads_sink_logits"], (plain_counts, counts)
    _same(tokens, want, f"{kind_name}: all -inf logits against the engine without the call")
    for item_id in want:
        for a, b in zip(figures[item_id], want_figures[item_id]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (kind_name, item_id, "prompt figures")
        for a, b in zip(chosen[item_id], want_chosen[item_id]):
            assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), (kind_name, item_id, "log-probabilities")


def test_set_sink_logits_refusals(mli, dev):
    import ctypes
    from min_llm_inference_amd import MliError
    _, items = _setup()

    def refused(fn, *needles):
        with pytest.raises(MliError) as err:
            fn()
        for needle in needles:
            assert needle in str(err.value), str(err.value)

    for kind in ("CONTIGUOUS", "PAGED_FP8"):
        e = _engine(kind)
        refused(lambda: e.set_sink_logits(Z), "mli_engine_set_sink_logits", "paged")
        e.close()
    for kind in KINDS:
        e = _engine(kind)
        refused(lambda: e.set_sink_logits(Z), "mli_engine_set_sink_logits", "n_heads must be >= 2")     # one head
        e.set_sink_logits(None)                                          # nothing to turn off: accepted
        e.set_heads(H)
        refused(lambda: e.set_sink_logits(Z[:2]), "mli_engine_set_sink_logits", "n must be the engine's n_heads (4)")
        refused(lambda: e.set_sink_logits(Z + (0.0,)), "mli_engine_set_sink_logits", "n_heads")
        for bad in (float("nan"), float("inf")):
            refused(lambda: e.set_sink_logits((0.0, bad, 0.0, 0.0)), "mli_engine_set_sink_logits", "finite or -inf")
        e.set_sink_logits((0.0, -float("inf"), -1e30, 1e30))             # -inf and both far logits: accepted
        e.set_sink_logits(Z)                                             # again, with other values: accepted before the start
        e.set_heads(H)                                                   # the same count: nothing to change
        refused(lambda: e.set_heads(2), "mli_engine_set_heads", "mli_engine_set_sink_logits")
        refused(lambda: e.set_heads(1), "mli_engine_set_sink_logits")
        refused(lambda: e.set_alibi(), "mli_engine_set_alibi", "mli_engine_set_sink_logits")
        refused(lambda: e.set_alibi([0.5] * H), "mli_engine_set_sink_logits")
        refused(lambda: e.set_softcap(2.0), "mli_engine_set_softcap", "mli_engine_set_sink_logits")
        e.set_softcap(0.0)                                               # no cap: nothing to refuse
        e.set_logprobs(2)
        e.set_prompt_logprobs(True)                                      # prompts are scored under the model that decodes
        e.set_kv_heads(2)                                                # every other option composes
        e.set_window(W)
        e.set_sinks(K)
        e.set_sink_logits(None)                                          # off again: ALiBi and the cap are free to come
        e.set_prompt_logprobs(False)
        e.set_alibi()
        refused(lambda: e.set_sink_logits(Z), "mli_engine_set_sink_logits", "ALiBi")       # the other order
        e.close()
        e = _engine(kind, n_heads=H, softcap=2.0)
        refused(lambda: e.set_sink_logits(Z), "mli_engine_set_sink_logits", "soft-capping")   # the other order
        e.set_softcap(0.0)
        e.set_sink_logits(Z)
        e.close()
        e = _engine(kind, n_heads=H, logprobs=0, prompt_logprobs=True)
        e.set_sink_logits(Z)                                             # after the prompt switch, too
        e.close()
    # lean layers only: with lean layers off an engine cannot have two heads (set_heads refuses them), so the setter on it is
    # refused for its one head; what is left to test is lean_layers = 0 AFTER the logits
    e = _engine("PAGED", n_heads=1)
    e.configure(lean_layers=False)
    refused(lambda: e.set_heads(H), "lean")
    refused(lambda: e.set_sink_logits(Z), "mli_engine_set_sink_logits", "n_heads must be >= 2")
    e.configure(lean_layers=True)
    e.set_heads(H)
    e.set_sink_logits(Z)
    refused(lambda: e.configure(lean_layers=False), "mli_engine_set_sink_logits", "lean")
    # after the first step the logits stay
    e.add_item(*items[0])
    e.step()
    refused(lambda: e.set_sink_logits(Z), "started")
    refused(lambda: e.set_sink_logits(None), "started")
    e.close()
    z = (ctypes.c_float * H)(*Z)
    assert mli.mli_engine_set_sink_logits(None, z, H) == -1 and b"null argument" in mli.mli_engine_last_error()
