"""Rotary position embeddings through the engine C ABI (mli_engine_set_rope / mli_engine_set_rope_table), on the pattern and at
the sizes of tests/test_alibi_engine_gpu.py: n_batch 8, n_sequence 64, emb_dim 128, n_vocab 1024, 16 items with prompts of
3 .. 20 tokens, the same model (its learned position table stays and is still added).
  - every token of every item of PAGED, PAGED_GEMM, PAGED_BF16 (both bf16 tile engines) and PAGED_FP8 (one head) is audited
    against the float64 replay with rotated q and stored K (tests/rope_model.audit: replay_model's rules, MASK_CAP included);
  - 4 heads on 4 and on 2 K/V heads; window + sinks + page release; half the pool (preemption: a re-admitted item is prefilled
    again at the same slots); n_forward_rounds 2; both loops; a step graph: scheduling never changes an item's tokens;
  - a table of all (1, 0) gives the tokens of the engine without the switch, the standard table gives others, and
    set_rope(theta) is set_rope_table(ops.rope_table(...));
  - the refusals of the two setters and of the setters that come after them."""
import functools

import numpy as np
import pytest

import gqa_model as gm
import replay_model as rm
import rope_model as rp
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, H, W, K = 8, 64, 128, 1024, 4, 12, 4
SEED, N_ITEMS = 8648, 16
WORST_CASE_BLOCKS = B * S // 16
KINDS = ["PAGED", "PAGED_GEMM", "PAGED_BF16"]
THETA = 10000.0


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(SEED, V, S, D), make_items(SEED + 1000, N_ITEMS, 3, 20)


def _engine(kind_name, **kw):
    from min_llm_inference_amd import engine as eng
    model, _ = _setup()
    kw.setdefault("n_blocks", 0 if kind_name == "CONTIGUOUS" else WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                      model["wv"], **kw)


def _run(kind_name, rope=THETA, heads=H, n_kv_heads=None, window=None, sinks=None, release=False, n_blocks=WORST_CASE_BLOCKS,
         rounds=1, pipelined=False, graphs=False, sampled=False, audit=True, logprobs=None, native=True):
    """rope: theta, a table, or None (the engine without the switch)"""
    model, items = _setup()
    n_kv_heads = n_kv_heads or heads
    e = _engine(kind_name, n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=heads, n_kv_heads=None if heads == 1 else n_kv_heads,
                window=window, sinks=sinks, release_pages=release, logprobs=logprobs, rope=rope)
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
    if audit and not sampled and rope is not None:
        table = rp.standard_table(S, D // heads, rope) if np.isscalar(rope) else np.asarray(rope, np.float32)
        plain = rm.spec_of_kind(kind_name, heads, window, (sinks or 0) if window is not None else 0, native=native)
        rp.audit(gm.expand_model(model, heads, n_kv_heads) if heads > 1 else model, items, finished, rp.rope_spec(plain, table), S,
                 total_tokens=st.total_tokens,
                 what=f"rope engine {kind_name} H {heads} Hkv {n_kv_heads}, {rounds} round(s), {n_blocks} pages, pipelined {pipelined}"
                 ).assert_ok()
    return out


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert len(got[k]) == len(want[k]) and (got[k] == want[k]).all(), (what, k)


def _differ(a, b):
    return any(len(a[k]) != len(b[k]) or (a[k] != b[k]).any() for k in a)


CONFIGS = [("PAGED", H, H, True), ("PAGED", H, 2, True), ("PAGED_GEMM", H, H, True), ("PAGED_GEMM", H, 2, True),
           ("PAGED_BF16", H, H, True), ("PAGED_BF16", H, 2, True), ("PAGED_BF16", H, 2, False), ("PAGED", 1, 1, True),
           ("PAGED_FP8", 1, 1, True)]


@pytest.mark.parametrize("kind_name,heads,n_kv_heads,native", CONFIGS,
                         ids=[f"{k}-H{h}-Hkv{kv}{'' if n else '-widened'}" for k, h, kv, n in CONFIGS])
def test_engine_with_rope_is_audited_and_independent_of_scheduling(mli, dev, kind_name, heads, n_kv_heads, native):
    from min_llm_inference_amd import ops
    try:
        assert mli.mli_tune(b"bf16_native_mfma", int(native)) == 0
        kw = dict(heads=heads, n_kv_heads=n_kv_heads, native=native)
        what = f"{kind_name}, {heads} head(s) on {n_kv_heads} K/V head(s), theta {THETA}"
        base = _run(kind_name, **kw)
        _same(_run(kind_name, pipelined=True, **kw), base, f"{what}: pipelined loop")
        _same(_run(kind_name, rounds=2, **kw), base, f"{what}: n_forward_rounds 2")
        _same(_run(kind_name, rounds=2, pipelined=True, **kw), base, f"{what}: n_forward_rounds 2, pipelined")
        _same(_run(kind_name, graphs=True, **kw), base, f"{what}: step graphs on a private stream")
        _same(_run(kind_name, n_blocks=WORST_CASE_BLOCKS // 2, **kw), base, f"{what}: half the pool (preemption)")
        _same(_run(kind_name, n_blocks=WORST_CASE_BLOCKS // 2, pipelined=True, **kw), base, f"{what}: half the pool, pipelined")
        _same(_run(kind_name, logprobs=2, **kw), base, f"{what}: with log-probabilities")
        _same(_run(kind_name, rope=ops.rope_table(S, D // heads, THETA), **kw), base, f"{what}: the same table through set_rope_table")
        plain = _run(kind_name, rope=None, **kw)
        assert _differ(plain, base), "set_rope is a no-op"
        _same(_run(kind_name, rope=rp.identity_table(S, D // heads), audit=False, **kw), plain,
              f"{what}: a table of all (1, 0) is the engine without the switch")
        other = _run(kind_name, rope=500000.0, **kw)
        assert _differ(other, base), "the engine ignores the theta it is given"
    finally:
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("kind_name,heads,n_kv_heads", [("PAGED", H, 2), ("PAGED_GEMM", H, 2), ("PAGED_BF16", H, 2), ("PAGED_FP8", 1, 1)])
def test_engine_with_rope_window_sinks_and_page_release(mli, dev, kind_name, heads, n_kv_heads):
    kw = dict(heads=heads, n_kv_heads=n_kv_heads, window=W, sinks=K)
    what = f"{kind_name}, {heads} head(s) on {n_kv_heads} K/V head(s), window {W}, {K} sinks, theta {THETA}"
    base = _run(kind_name, **kw)
    _same(_run(kind_name, release=True, **kw), base, f"{what}: release_pages")
    _same(_run(kind_name, release=True, pipelined=True, rounds=2, **kw), base, f"{what}: release_pages, pipelined, n_forward_rounds 2")
    _same(_run(kind_name, release=True, n_blocks=WORST_CASE_BLOCKS // 2, graphs=True, **kw), base,
          f"{what}: release_pages, half the pool, step graphs")
    assert _differ(_run(kind_name, heads=heads, n_kv_heads=n_kv_heads), base), "the window is a no-op beside the rotation"
    assert _differ(_run(kind_name, rope=None, **kw), base), "the rotation is a no-op beside the window"


def test_rope_composes_with_alibi_and_sampling(mli, dev):
    from min_llm_inference_amd import engine as eng
    model, items = _setup()

    def run(rope, alibi, sampled=False, pipelined=False, n_blocks=WORST_CASE_BLOCKS):
        e = eng.Engine(eng.PAGED_BF16, B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"], model["wv"],
                       n_blocks=n_blocks, n_heads=H, n_kv_heads=2, alibi=alibi, rope=rope)
        e.set_pipelined(pipelined)
        for item_id, toks in items:
            e.add_item(item_id, toks, **(dict(temperature=0.8, top_p=0.95, seed=4000 + item_id) if sampled else {}))
        st = e.run()
        out = dict(e.finished())
        e.close()
        assert st.finished == len(items)
        return out

    both = run(THETA, True)
    _same(run(THETA, True, pipelined=True, n_blocks=WORST_CASE_BLOCKS // 2), both, "RoPE + ALiBi: half the pool, pipelined")
    assert _differ(both, run(THETA, None)) and _differ(both, run(None, True)), "one of the two is dropped beside the other"
    a = run(THETA, None, sampled=True)
    _same(run(THETA, None, sampled=True), a, "sampled run, again")
    _same(run(THETA, None, sampled=True, pipelined=True), a, "sampled run, pipelined loop")
    assert _differ(a, run(None, None, sampled=True)), "the sampled run ignores the rotation"


def test_set_rope_refusals(mli, dev):
    from min_llm_inference_amd import MliError
    _, items = _setup()

    def refused(fn, *needles):
        with pytest.raises(MliError) as err:
            fn()
        for needle in needles:
            assert needle in str(err.value), str(err.value)

    assert mli.mli_engine_set_rope(None, 10000.0) == -1 and b"null argument" in mli.mli_engine_last_error()
    assert mli.mli_engine_set_rope_table(None, None, 0) == -1 and b"null argument" in mli.mli_engine_last_error()
    e = _engine("CONTIGUOUS")
    refused(lambda: e.set_rope(), "mli_engine_set_rope", "paged")
    refused(lambda: e.set_rope(rp.identity_table(S, D)), "mli_engine_set_rope_table", "paged")
    e.close()
    for kind in KINDS + ["PAGED_FP8"]:
        heads = 1 if kind == "PAGED_FP8" else H
        hd = D // heads
        e = _engine(kind, n_heads=heads)
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            refused(lambda: e.set_rope(bad), "theta")
        good = rp.standard_table(S, hd)
        for bad in (good[:-1], np.concatenate([good, good[:1]]), rp.standard_table(S, hd * 2), good[:, :-1]):
            refused(lambda: e.set_rope(bad), "n_floats")                       # a wrong count
        for bad in (float("nan"), float("inf"), -float("inf")):
            t = good.copy()
            t[S // 2, 3, 1] = bad
            refused(lambda: e.set_rope(t), "finite")
        assert mli.mli_engine_set_rope_table(e._h, None, S * hd) == -1 and b"null argument" in mli.mli_engine_last_error()
        e.set_rope()
        e.set_rope(good)                                                       # again, with a table: accepted before the start
        if kind != "PAGED_FP8":
            e.set_heads(heads)                                                 # the same count: nothing to change
            refused(lambda: e.set_heads(2), "mli_engine_set_rope")             # the table is that of 4 heads
            e.set_logprobs(2)
            refused(lambda: e.set_prompt_logprobs(True), "RoPE")
            e.set_kv_heads(2)                                                  # every other option composes
            e.set_alibi()
        e.set_window(W)
        e.set_sinks(K)
        e.set_page_release(True)
        refused(lambda: e.configure(lean_layers=False), "lean")
        e.add_item(*items[0])
        e.step()
        refused(lambda: e.set_rope(), "started")
        refused(lambda: e.set_rope(good), "started")
        e.close()
    for kind in KINDS:
        e = _engine(kind, n_heads=H, logprobs=0, prompt_logprobs=True)
        refused(lambda: e.set_rope(), "prompt")
        refused(lambda: e.set_rope(rp.standard_table(S, D // H)), "prompt")
        e.close()
    e = _engine("PAGED", n_heads=1)                                            # lean layers off first
    e.configure(lean_layers=False)
    refused(lambda: e.set_rope(), "mli_engine_set_rope", "lean")
    refused(lambda: e.set_rope(rp.standard_table(S, D)), "mli_engine_set_rope_table", "lean")
    e.close()
