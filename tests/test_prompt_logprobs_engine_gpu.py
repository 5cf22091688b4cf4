"""The prompt log-probabilities the engines report (mli_engine_set_prompt_logprobs), held to the float64 replay of
tests/replay_model.py: the teacher-forced forward that audits every emitted token also gives the logits of the prompt positions
(rows 0 .. p - 2: position i chooses token i + 1).

Shape replay_model.SAMPLED_SHAPE (n_batch 8, n_sequence 128, emb_dim 128, n_vocab 1024), its 16 items (prompts of 3 .. 60
tokens: most are longer than n_batch positions and take several passes), n_top 3, all greedy and the "top-p" workload, on:
PAGED pipelined with half the worst-case pool (preemption: every item is still scored exactly once) and sequential; PAGED_GEMM
with step graphs; PAGED_BF16 with 2 rounds; PAGED_GEMM with 4 heads under window 40 plus 4 sinks; PAGED_BF16 with 4 heads on 2
K/V heads.

  unchanged    tokens and generated-token figures bit-identical to the same engine without prompt_logprobs
  bound        per item 2 (tol_logit + E_flip) + tol_lse over the PROMPT rows (prompt_model.prompt_bound): the float32
               restatement's error against the float64 forward, as replay_model.judge_item takes it over the generated rows;
               nothing comes from a kernel
  figures      n_scored == n_prompt - 1; |token_logprob - the replay's logprob of prompt token i + 1| <= bound; the conditions
               on the alternatives of tests/test_logprobs_engine_gpu.py
  continuity   an item whose prompt is another item's finished stream reports, at that stream's generated positions, prompt
               figures within twice the bound of what the first item reported when it generated them"""
import functools

import numpy as np
import pytest

import gqa_model as gm
import prompt_model as pm
import replay_model as rm
from test_logprobs_engine_gpu import FULL, N_TOP, SHAPE, _workload

pytestmark = pytest.mark.gpu

CASES = {
    "PAGED, pipelined, half the pool": dict(kind="PAGED", n_blocks=FULL // 2, pipelined=True),
    "PAGED, sequential": dict(kind="PAGED", n_blocks=FULL),
    "PAGED_GEMM, step graphs": dict(kind="PAGED_GEMM", n_blocks=FULL, graphs=True),
    "PAGED_BF16, 2 rounds": dict(kind="PAGED_BF16", n_blocks=FULL, rounds=2, pipelined=True),
    "PAGED_GEMM, 4 heads, window 40, 4 sinks": dict(kind="PAGED_GEMM", n_blocks=FULL, pipelined=True, n_heads=4,
                                                   window=rm.SAMPLED_SHAPE["W"], sinks=4),
    "PAGED_BF16, 4 heads on 2 K/V heads": dict(kind="PAGED_BF16", n_blocks=FULL, pipelined=True, n_heads=4, n_kv_heads=2),
}


def _engine(eng, model, kind, n_blocks, rounds=1, n_heads=1, window=None, sinks=None, n_kv_heads=None, logprobs=N_TOP,
            prompt=False, **_):
    return eng.Engine(getattr(eng, kind), SHAPE["B"], SHAPE["S"], SHAPE["D"], SHAPE["V"], model["emb_table"], model["pos_table"],
                      model["wk"], model["wq"], model["wv"], n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=n_heads,
                      window=window, sinks=sinks, n_kv_heads=n_kv_heads, logprobs=logprobs, prompt_logprobs=prompt)


def _run(model, items, sampling, prompt, case):
    from min_llm_inference_amd import engine as eng
    e = _engine(eng, model, prompt=prompt, **case)
    try:
        if case.get("graphs"):
            e.use_private_stream()
            e.configure(step_graphs=True)
        e.set_pipelined(bool(case.get("pipelined")))
        for item_id, toks in items:
            if sampling and item_id in sampling:
                T, top_k, top_p, seed = sampling[item_id]
                e.add_item(item_id, toks, temperature=T, top_k=top_k, top_p=top_p, seed=seed)
            else:
                e.add_item(item_id, toks)
        e.run()
        return (dict(e.finished()), e.finished_logprobs(), e.finished_prompt_logprobs() if prompt else None,
                e.page_stats().preemptions)
    finally:
        e.close()


def _replay_model(model, case):
    H, Hkv = case.get("n_heads", 1), case.get("n_kv_heads")
    return gm.expand_model(model, H, Hkv) if Hkv else model


def _judge(what, model, case, items, finished, figures):
    """The prompt figures of one run against the replay; returns {id: bound}."""
    spec = rm.spec_of_kind(case["kind"], case.get("n_heads", 1), case.get("window"), case.get("sinks") or 0)
    model = _replay_model(model, case)
    bounds, worst_ratio, worst, worst_bound = {}, 0.0, 0.0, 0.0
    for item_id, prompt in items:
        p = len(prompt)
        lp, ids, tops = figures[item_id]
        assert len(lp) == p - 1 and ids.shape == (p - 1, N_TOP) and tops.shape == (p - 1, N_TOP), (what, item_id, len(lp), p)
        if p < 2:
            continue
        toks = np.asarray(finished[item_id])
        rep = pm.prompt_replay(model, toks, p, spec)
        bound, _ = pm.prompt_bound(rep)
        bounds[item_id] = bound
        lg = rep.logits
        m = lg.max(axis=1, keepdims=True)
        lp64 = lg - m - np.log(np.exp(lg - m).sum(axis=1, keepdims=True))
        given = pm.prompt_targets(toks, p - 1)
        assert (given == np.asarray(prompt)[1:]).all()
        e_tok = np.abs(lp.astype(np.float64) - lp64[np.arange(p - 1), given])
        assert (ids >= 0).all() and (ids < SHAPE["V"]).all(), item_id
        e_top = np.abs(tops.astype(np.float64) - np.take_along_axis(lp64, ids.astype(np.int64), axis=1))
        err = max(float(e_tok.max()), float(e_top.max()))
        assert err <= bound, f"{what}: item {item_id}: a prompt logprob is {err:.3e} from the replay's, bound {bound:.3e}"
        unreported = lg.copy()
        np.put_along_axis(unreported, ids.astype(np.int64), -np.inf, axis=1)
        beats = unreported.max(axis=1) - np.take_along_axis(lg, ids[:, -1:].astype(np.int64), axis=1)[:, 0]
        assert beats.max() <= 2 * bound, f"{what}: item {item_id}: an unreported id beats the last alternative by {beats.max():.3e}"
        assert (np.diff(np.take_along_axis(lg, ids.astype(np.int64), axis=1), axis=1) <= 2 * bound).all(), item_id
        assert np.exp(tops.astype(np.float64)).sum(axis=1).max() <= 1 + bound, item_id
        hit = ids == given[:, None]                                            # the token among its alternatives: the same bits
        assert (tops[hit].view(np.uint32) == np.broadcast_to(lp[:, None], tops.shape)[hit].view(np.uint32)).all(), item_id
        if err / bound >= worst_ratio:
            worst, worst_bound, worst_ratio = err, bound, err / bound
    print(f"PROMPT LOGPROBS engine {what}: worst error {worst:.3e} against bound {worst_bound:.3e} (ratio {worst_ratio:.3g})")
    return bounds


@pytest.mark.parametrize("which", ["greedy", "top-p"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_engine_prompt_logprobs_match_the_replay_and_change_nothing_else(mli, dev, name, which):
    case = CASES[name]
    model, items, sampling = _workload(which)
    assert max(len(t) for _, t in items) - 1 > SHAPE["B"], "a prompt longer than one pass"
    fin0, fig0, _, _ = _run(model, items, sampling, False, case)
    fin1, fig1, prompt_figures, preemptions = _run(model, items, sampling, True, case)
    if "half the pool" in name:
        assert preemptions > 0, "the pool was meant to run dry"
    assert sorted(fin1) == sorted(fin0) == sorted(i for i, _ in items)
    for item_id, _ in items:
        assert np.array_equal(fin1[item_id], fin0[item_id]), (name, item_id)
        for a, b in zip(fig1[item_id][1:], fig0[item_id][1:]):
            assert a.tobytes() == b.tobytes(), (name, item_id, "generated-token figures changed")
        assert fig1[item_id][0] == fig0[item_id][0]
    assert sorted(prompt_figures) == sorted(fin1), "every item is scored exactly once"
    _judge(f"{name}, {which}", model, case, items, fin1, prompt_figures)


@pytest.mark.parametrize("name", ["PAGED, sequential", "PAGED_BF16, 2 rounds"])
def test_a_finished_stream_scored_as_a_prompt_agrees_with_the_figures_it_was_generated_with(mli, dev, name):
    case = CASES[name]
    model, items, _ = _workload("greedy")
    S = SHAPE["S"]
    fin, fig, first_prompt, _ = _run(model, items, None, True, case)
    bounds = _judge(f"{name}, first run", model, case, items, fin, first_prompt)
    again = [(item_id, np.asarray(fin[item_id][:S - 1], np.int32)) for item_id, _ in items]
    fin2, _, second_prompt, _ = _run(model, again, None, True, case)
    bounds2 = _judge(f"{name}, finished streams as prompts", model, case, again, fin2, second_prompt)
    worst, checked = 0.0, 0
    for item_id, prompt in items:
        p = len(prompt)
        n_prompt, lp, _, _ = fig[item_id]
        assert n_prompt == p
        lp2 = second_prompt[item_id][0]
        n = min(len(lp), len(lp2) - (p - 1))                 # generated position p + r is prompt entry p + r - 1 of the second run
        assert n >= 1
        d = np.abs(lp[:n].astype(np.float64) - lp2[p - 1:p - 1 + n])
        bound = max(bounds.get(item_id, 0.0), bounds2[item_id])
        worst = max(worst, float(d.max()) / bound)
        checked += n
        assert d.max() <= 2 * bound, (name, item_id, float(d.max()), bound)
    print(f"PROMPT LOGPROBS continuity {name}: {checked} positions, at most {worst:.3g} bounds apart")


def test_refusals_on_a_live_device(mli, dev):
    from min_llm_inference_amd import engine as eng
    model, items, _ = _workload("greedy")

    def make(kind, **kw):
        return _engine(eng, model, kind=kind, n_blocks=0 if kind == "CONTIGUOUS" else FULL, **kw)

    for kind, kw, match in (("PAGED", dict(logprobs=None), "logprobs"), ("CONTIGUOUS", {}, "paged"), ("PAGED_FP8", {}, "paged")):
        e = make(kind, **kw)
        try:
            with pytest.raises(eng.MliError, match=match):
                e.set_prompt_logprobs(True)
        finally:
            e.close()
    e = make("PAGED", window=40)
    try:
        e.set_page_release(True)
        with pytest.raises(eng.MliError, match="release"):
            e.set_prompt_logprobs(True)
    finally:
        e.close()
    e = make("PAGED", window=40)
    try:
        e.set_prompt_logprobs(True)
        with pytest.raises(eng.MliError, match="prompt"):
            e.set_page_release(True)
    finally:
        e.close()
    e = make("PAGED")                                           # a started engine
    try:
        e.add_item(*items[0])
        e.set_pipelined(False)
        e.step()
        with pytest.raises(eng.MliError, match="started"):
            e.set_prompt_logprobs(True)
    finally:
        e.close()
    wide = eng.Engine(eng.PAGED, 2, 64, 1024, 1024, np.zeros((1024, 1024), np.float32), np.zeros((64, 1024), np.float32),
                      *(np.zeros((1024, 1024), np.float32) for _ in range(3)), n_blocks=8, logprobs=0)
    try:
        with pytest.raises(eng.MliError, match="lane loads"):     # fp32 rows of four lane loads
            wide.set_prompt_logprobs(True)
    finally:
        wide.close()
    e = make("PAGED", logprobs=0)                               # n_top 0 and a one-token prompt: no figures, an empty record
    try:
        e.set_prompt_logprobs(True)
        e.add_item(77, np.asarray([5], np.int32))
        e.add_item(78, np.asarray([5, 6], np.int32))
        e.run()
        got = e.finished_prompt_logprobs()
        assert len(got[77][0]) == 0 and len(got[78][0]) == 1 and got[78][1].shape == (1, 0)
    finally:
        e.close()
