"""mli_engine_set_heads_mfma_f32: tests/test_gqa_mfma_engine_gpu.py's engine (emb_dim 2048, 16 heads of 128 on 4 K/V heads, B 4,
S 64) on the fp32 paged kinds, which mli_engine_set_heads refuses at this width; every token audited against the float64 replay
on the expanded model.  The pool of 5 pages must preempt: only an engine that releases pages below its window runs dry here."""
import functools

import pytest

import gqa_model as gm
import replay_model as rm
import rope_model as rp
from engine_sim import make_items, make_model

pytestmark = pytest.mark.gpu

B, S, D, V, H, HKV, W = 4, 64, 2048, 1024, 16, 4, 12
SEED, N_ITEMS, THETA, WORST_CASE_BLOCKS = 8650, 10, 10000.0, B * S // 16


@functools.lru_cache(maxsize=2)
def _setup(emb_dim=D):
    model = make_model(SEED, V, S, emb_dim)
    return model, gm.expand_model(model, H, HKV) if emb_dim == D else None, make_items(SEED + 1000, N_ITEMS, 3, 20)


def _engine(kind_name="PAGED", emb_dim=D, **kw):
    from min_llm_inference_amd import engine as eng
    model = _setup(emb_dim)[0]
    kw.setdefault("n_blocks", 0 if kind_name == "CONTIGUOUS" else WORST_CASE_BLOCKS)
    return eng.Engine(getattr(eng, kind_name), B, S, emb_dim, V, model["emb_table"], model["pos_table"], model["wk"],
                      model["wq"], model["wv"], **kw)


RUNS = {   # kind, window, release_pages, rope, pipelined, n_blocks
    "plain": ("PAGED", None, False, None, False, WORST_CASE_BLOCKS),
    "gemm-plain": ("PAGED_GEMM", None, False, None, False, WORST_CASE_BLOCKS),
    "window-release": ("PAGED", W, True, None, False, WORST_CASE_BLOCKS),
    "rope": ("PAGED", None, False, THETA, False, WORST_CASE_BLOCKS),
    "preempted-pipelined": ("PAGED", W, True, None, True, 5),
}


@pytest.mark.parametrize("name", list(RUNS))
def test_f32_engine_on_the_mfma_scan_is_audited(mli, dev, name):
    from min_llm_inference_amd import ops
    kind, window, release, rope, pipelined, n_blocks = RUNS[name]
    _, expanded, items = _setup()
    e = _engine(kind, n_blocks=n_blocks, n_heads=H, n_kv_heads=HKV, heads_mfma=True, window=window, release_pages=release, rope=rope)
    e.set_pipelined(pipelined)
    for item_id, toks in items:
        e.add_item(item_id, toks)
    ops.reset_launch_counts()
    st = e.run()
    finished, pages = e.finished(), e.page_stats()
    e.close()
    assert st.finished == len(items)
    scans = {f: ops.launch_count(f) for f in ops.launch_families() if f.startswith("scan_") and ops.launch_count(f)}
    assert list(scans) == ["scan_gqa_mfma_f32"], scans
    assert (pages.preemptions > 0) == (n_blocks < WORST_CASE_BLOCKS), pages.preemptions
    spec, what = rm.spec_of_kind(kind, H, window, 0), dict(total_tokens=st.total_tokens, what=f"gqa mfma f32 engine, {name}")
    if rope is None:
        rm.audit(expanded, items, finished, spec, S, **what).assert_ok()
    else:
        rp.audit(expanded, items, finished, rp.rope_spec(spec, rp.standard_table(S, D // H, rope)), S, **what).assert_ok()


# name -> (kind, emb_dim, calls before, the refused call, what its message holds).  SMALL: D 256, a width every other setter takes
NAME, MFMA, SMALL = "mli_engine_set_heads_mfma_f32", (lambda e: e.set_heads_mfma_f32(H, HKV)), (lambda e: e.set_heads_mfma_f32(4, 2))
LANES = [lambda e: e.set_heads(4), lambda e: e.set_window(W)]
EXCLUDED = {"sinks": (lambda e: e.set_sinks(4), "sink tokens"), "alibi": (lambda e: e.set_alibi(), "ALiBi"),
            "softcap": (lambda e: e.set_softcap(30.0), "soft-capping"),
            "sink_logits": (lambda e: e.set_sink_logits([0.5] * 4), "sink logits"),
            "prompt_logprobs": (lambda e: (e.set_logprobs(0), e.set_prompt_logprobs(True)), "prompt log-probabilities")}
REFUSALS = {f"after the switch: {k}, {kind}": (kind, 256, [SMALL], f, (NAME, "MFMA"))
            for k, (f, _) in EXCLUDED.items() for kind in ("PAGED", "PAGED_GEMM")}
REFUSALS.update({f"before the switch: {k}": ("PAGED", 256, LANES + [f], SMALL, (NAME, needle)) for k, (f, needle) in EXCLUDED.items()})
REFUSALS.update({f"kind {k}": (k, D, [], MFMA, (NAME, "fp32 paged engines")) for k in ("CONTIGUOUS", "PAGED_BF16", "PAGED_FP8")})
REFUSALS.update({
    **{what: ("PAGED", D, [], lambda e, h=h, k=k: e.set_heads_mfma_f32(h, k), (NAME, needle)) for what, h, k, needle in (
        ("divisor", H, 3, "divide"), ("head_dim 32", 64, 64, "unsupported"), ("head_dim 256", 8, 8, "unsupported"), ("group 16", H, 1, "unsupported"))},
    "lane-group heads at this width": ("PAGED", D, [], lambda e: e.set_heads(H), ("mli_engine_set_heads",)),
    "set_heads": ("PAGED_GEMM", D, [MFMA], lambda e: e.set_heads(8), (NAME, "call it again")),
    "lean layers": ("PAGED", D, [MFMA], lambda e: e.configure(lean_layers=False), (NAME, "lean")),
    "started": ("PAGED", D, [MFMA, lambda e: e.add_item(*_setup()[2][0]), lambda e: e.step()], MFMA, (NAME, "started")),
})


@pytest.mark.parametrize("name", list(REFUSALS))
def test_set_heads_mfma_f32_refusals(mli, dev, name):
    from min_llm_inference_amd import MliError
    kind, emb_dim, before, refused, needles = REFUSALS[name]
    e = _engine(kind, emb_dim)
    for call in before:
        call(e)
    with pytest.raises(MliError) as err:
        refused(e)
    e.close()
    assert all(needle in str(err.value) for needle in needles), str(err.value)
