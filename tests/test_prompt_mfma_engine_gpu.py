"""mli_engine_set_prompt_mfma: a PAGED_BF16 engine at emb_dim 512, 8 heads of 64 on 2 K/V heads, n_batch 4, n_sequence 64, 10 items
with prompts of 3 .. 20 tokens, logprobs and prompt logprobs, plain and under a window.  With the switch, tokens and generated-token
figures are bit-identical to the engine without it, every prompt figure lies within prompt_model.prompt_bound of the float64
replay, and "scan_prompt_mfma" is the only prompt family counted.  The setter's refusals, in both call orders."""
import functools

import numpy as np
import pytest

import gqa_model as gm
import prompt_model as pm
import replay_model as rm
from engine_sim import make_items, make_model
from test_gqa_mfma_engine_gpu import _refused

pytestmark = pytest.mark.gpu

B, S, D, V, H, HKV, W, N_TOP = 4, 64, 512, 1024, 8, 2, 12, 2
SEED, N_ITEMS = 8731, 10


@functools.lru_cache(maxsize=1)
def _setup():
    model = make_model(SEED, V, S, D)
    return model, gm.expand_model(model, H, HKV), make_items(SEED + 1000, N_ITEMS, 3, 20)


def _engine(kind_name="PAGED_BF16", **kw):
    from min_llm_inference_amd import engine as eng
    model = _setup()[0]
    kw.setdefault("n_blocks", 0 if kind_name == "CONTIGUOUS" else B * S // 16)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


def _run(window, prompt_mfma):
    from min_llm_inference_amd import ops
    e = _engine(n_heads=H, n_kv_heads=HKV, window=window, logprobs=N_TOP, prompt_logprobs=True, prompt_mfma=prompt_mfma)
    for item_id, toks in _setup()[2]:
        e.add_item(item_id, toks)
    ops.reset_launch_counts()
    st = e.run()
    out = dict(e.finished()), e.finished_logprobs(), e.finished_prompt_logprobs()
    e.close()
    assert st.finished == N_ITEMS
    prompt = {f for f in ops.launch_families() if f.startswith("scan_prompt") and ops.launch_count(f)}
    assert prompt == {"scan_prompt_mfma" if prompt_mfma else "scan_prompt"}, prompt
    return out


@pytest.mark.parametrize("window", [None, W])
def test_engine_with_the_prompt_mfma_switch(mli, dev, window):
    _, expanded, items = _setup()
    try:
        assert mli.mli_tune(b"bf16_native_mfma", 0) == 0     # (the replay's bound is stated for the widened projection)
        tokens, gen, figures = _run(window, True)
        tokens0, gen0, _ = _run(window, False)
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)
    assert sorted(tokens) == sorted(tokens0) == sorted(figures)
    for item_id in tokens:
        assert np.array_equal(tokens[item_id], tokens0[item_id]), f"item {item_id}: the switch changed a token"
        assert gen[item_id][0] == gen0[item_id][0] and all(a.tobytes() == b.tobytes() for a, b in zip(gen[item_id][1:], gen0[item_id][1:])), \
            f"item {item_id}: the switch changed a generated token's figures"
    spec = rm.spec_of_kind("PAGED_BF16", H, window, 0)
    worst = 0.0
    for item_id, prompt in items:
        p = len(prompt)
        lp, ids, tops = figures[item_id]
        assert len(lp) == p - 1 and ids.shape == tops.shape == (p - 1, N_TOP), (item_id, len(lp), p)
        toks = np.asarray(tokens[item_id])
        rep = pm.prompt_replay(expanded, toks, p, spec)
        bound, _ = pm.prompt_bound(rep)
        lg = rep.logits
        m = lg.max(axis=1, keepdims=True)
        lp64 = lg - m - np.log(np.exp(lg - m).sum(axis=1, keepdims=True))
        e_tok = np.abs(lp.astype(np.float64) - lp64[np.arange(p - 1), pm.prompt_targets(toks, p - 1)])
        e_top = np.abs(tops.astype(np.float64) - np.take_along_axis(lp64, ids.astype(np.int64), axis=1))
        err = max(float(e_tok.max()), float(e_top.max()))
        assert err <= bound, f"item {item_id}: a prompt logprob is {err:.3e} from the replay's, bound {bound:.3e}"
        worst = max(worst, err / bound)
    print(f"PROMPT MFMA engine W {window}: worst prompt figure error {worst:.3g} of the bound")


# what the kernel does not have: (the setter, what the refusal names)
EXCLUDED = {"sinks": (lambda e: e.set_sinks(4), "sink tokens"), "softcap": (lambda e: e.set_softcap(30.0), "soft-capping"),
            "sink_logits": (lambda e: e.set_sink_logits([0.5] * H), "sink logits")}


@pytest.mark.parametrize("name", list(EXCLUDED))
def test_the_switch_and_what_it_excludes_refuse_each_other_in_both_orders(mli, dev, name):
    setter, needle = EXCLUDED[name]
    e = _engine(n_heads=H, n_kv_heads=HKV, window=W, logprobs=0, prompt_logprobs=True, prompt_mfma=True)
    _refused(lambda: setter(e), "mli_engine_set_prompt_mfma")
    e.close()
    e = _engine(n_heads=H, n_kv_heads=HKV, window=W, logprobs=0, prompt_logprobs=True)
    setter(e)
    _refused(lambda: e.set_prompt_mfma(True), "mli_engine_set_prompt_mfma", needle)
    e.close()


def test_set_prompt_mfma_refusals(mli, dev):
    # another kind | no prompt log-probabilities | head_dim 32
    for kind, kw, needle in (("PAGED", {}, "bf16 paged engine"), ("PAGED_FP8", {}, "bf16 paged engine"), ("CONTIGUOUS", {}, "bf16 paged engine"),
                             ("PAGED_BF16", dict(n_heads=H, n_kv_heads=HKV), "mli_engine_set_prompt_logprobs"),
                             ("PAGED_BF16", dict(n_heads=16, logprobs=0, prompt_logprobs=True), "unsupported")):
        e = _engine(kind, **kw)
        _refused(lambda: e.set_prompt_mfma(True), "mli_engine_set_prompt_mfma", needle)
        e.close()
    e = _engine(n_heads=H, n_kv_heads=HKV, logprobs=0, prompt_logprobs=True, prompt_mfma=True)
    e.add_item(*_setup()[2][0])
    e.step()
    _refused(lambda: e.set_prompt_mfma(True), "mli_engine_set_prompt_mfma", "started")
    e.close()
