"""The log-probabilities the engines report (mli_engine_set_logprobs), held to the float64 replay of
tests/replay_model.py: the same teacher-forced forward that audits every emitted token also gives the logits behind it, so a
reported figure is judged by the model that judges its token.

Shape replay_model.SAMPLED_SHAPE (n_batch 8, n_sequence 128, emb_dim 128, n_vocab 1024), 16 items, all greedy and the "top-p"
sampled workload (half the items drawn at T 0.8, top_p 0.95), n_top 3, on: PAGED pipelined with half the worst-case pool
(preemption) and sequential; PAGED_GEMM with step graphs; PAGED_BF16 with 2 rounds; PAGED_FP8; CONTIGUOUS; PAGED_GEMM with 4
heads under window 40 plus 4 sinks.

  tokens       those of the same engine without logprobs; n_generated == n_tokens - n_prompt for every item
  bound        per item, 2 (tol_logit + E_flip) + tol_lse: tol_logit and E_flip are the replay audit's own figures for the item
               (an LSE moves at most as far as its logits, the token's logit as far again), tol_lse the float32 restatement's
               bound on the replay's logits (logprobs_model.tolerance); nothing comes from a kernel
  token        |token_logprob - the replay's logprob of that token| <= bound
  alternatives every reported id's logprob within the bound of the replay's for that id; no unreported id beats the last
               reported one by more than twice the bound; sum exp(top_logprobs) <= 1 + bound
  loops        the pipelined and the sequential loop agree within twice the bound (not bit for bit: the equal-shares scan's
               summation order depends on the batch)"""
import functools

import numpy as np
import pytest

import logprobs_model as lm
import replay_model as rm

pytestmark = pytest.mark.gpu

N_TOP = 3
SHAPE = {k: rm.SAMPLED_SHAPE[k] for k in ("B", "S", "D", "V")}
FULL = SHAPE["B"] * SHAPE["S"] // 16

CASES = {
    "PAGED, pipelined, half the pool": dict(kind="PAGED", n_blocks=FULL // 2, pipelined=True),
    "PAGED, sequential": dict(kind="PAGED", n_blocks=FULL),
    "PAGED_GEMM, step graphs": dict(kind="PAGED_GEMM", n_blocks=FULL, graphs=True),
    "PAGED_BF16, 2 rounds": dict(kind="PAGED_BF16", n_blocks=FULL, rounds=2, pipelined=True),
    "PAGED_FP8": dict(kind="PAGED_FP8", n_blocks=FULL, pipelined=True),
    "CONTIGUOUS": dict(kind="CONTIGUOUS", n_blocks=0),
    "PAGED_GEMM, 4 heads, window 40, 4 sinks": dict(kind="PAGED_GEMM", n_blocks=FULL, pipelined=True, n_heads=4,
                                                   window=rm.SAMPLED_SHAPE["W"], sinks=4),
}


@functools.lru_cache(maxsize=None)
def _workload(which):
    model, items, sampling = rm.sampled_workload("top-p")
    return model, items, (sampling if which == "top-p" else None)


def _run(which, logprobs, kind, n_blocks, rounds=1, pipelined=False, graphs=False, n_heads=1, window=None, sinks=None):
    from min_llm_inference_amd import engine as eng
    model, items, sampling = _workload(which)
    k = getattr(eng, kind)
    e = eng.Engine(k, SHAPE["B"], SHAPE["S"], SHAPE["D"], SHAPE["V"], model["emb_table"], model["pos_table"], model["wk"],
                   model["wq"], model["wv"], n_blocks=n_blocks, n_forward_rounds=rounds, n_heads=n_heads, window=window,
                   sinks=sinks, logprobs=logprobs)
    try:
        if graphs:
            e.use_private_stream()
            e.configure(step_graphs=True)
        if k != eng.CONTIGUOUS:
            e.set_pipelined(bool(pipelined))
        for item_id, toks in items:
            if sampling and item_id in sampling:
                T, top_k, top_p, seed = sampling[item_id]
                e.add_item(item_id, toks, temperature=T, top_k=top_k, top_p=top_p, seed=seed)
            else:
                e.add_item(item_id, toks)
        st = e.run()
        preemptions = e.page_stats().preemptions if k != eng.CONTIGUOUS else 0
        return st, dict(e.finished()), (e.finished_logprobs() if logprobs is not None else None), preemptions
    finally:
        e.close()


def _judge(what, which, case, finished, figures):
    """The figures of one run against the replay; returns {id: bound} and prints the worst error / bound."""
    model, items, _ = _workload(which)
    spec = rm.spec_of_kind(case["kind"], case.get("n_heads", 1), case.get("window"), case.get("sinks") or 0)
    key = rm._fingerprint(model)
    bounds, worst, worst_bound, worst_ratio = {}, 0.0, 0.0, 0.0
    for item_id, prompt in items:
        toks = finished[item_id]
        n_prompt, lp, ids, tops = figures[item_id]
        p, n = len(prompt), len(toks)
        assert n_prompt == p and len(lp) == n - p and ids.shape == (n - p, N_TOP) and tops.shape == (n - p, N_TOP), item_id
        rep = rm.Replay(model, toks, spec, rows=np.arange(p - 1, n - 1))
        lg = rep.logits                                                       # lg[r] chose toks[p + r]
        m = lg.max(axis=1, keepdims=True)
        lp64 = lg - m - np.log(np.exp(lg - m).sum(axis=1, keepdims=True))
        j = rm.judge_item(model, p, toks, spec, None, rm.FLIP_ROUNDS, key)    # tol = 2 (tol_logit + E_flip)
        bound = j["tol"] + lm.tolerance(lg.astype(np.float32))
        bounds[item_id] = bound
        r = np.arange(n - p)
        e_tok = np.abs(lp.astype(np.float64) - lp64[r, toks[p:]])
        assert (ids >= 0).all() and (ids < SHAPE["V"]).all(), item_id
        e_top = np.abs(tops.astype(np.float64) - np.take_along_axis(lp64, ids.astype(np.int64), axis=1))
        err = max(float(e_tok.max()), float(e_top.max()))
        assert err <= bound, f"{what}: item {item_id}: a logprob is {err:.3e} from the replay's, bound {bound:.3e}"
        unreported = lg.copy()
        np.put_along_axis(unreported, ids.astype(np.int64), -np.inf, axis=1)
        beats = unreported.max(axis=1) - np.take_along_axis(lg, ids[:, -1:].astype(np.int64), axis=1)[:, 0]
        assert beats.max() <= 2 * bound, f"{what}: item {item_id}: an unreported id beats the last alternative by {beats.max():.3e}"
        assert (np.diff(np.take_along_axis(lg, ids.astype(np.int64), axis=1), axis=1) <= 2 * bound).all(), item_id
        assert np.exp(tops.astype(np.float64)).sum(axis=1).max() <= 1 + bound, item_id
        hit = ids == toks[p:, None]                                           # the token among its alternatives: the same bits
        assert (tops[hit].view(np.uint32) == np.broadcast_to(lp[:, None], tops.shape)[hit].view(np.uint32)).all(), item_id
        if err / bound >= worst_ratio:
            worst, worst_bound, worst_ratio = err, bound, err / bound
    print(f"LOGPROBS engine {what}: worst error {worst:.3e} against bound {worst_bound:.3e} (ratio {worst_ratio:.3g})")
    return bounds


@pytest.mark.parametrize("which", ["greedy", "top-p"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_engine_logprobs_match_the_replay(mli, dev, name, which):
    case = CASES[name]
    st0, plain, _, _ = _run(which, None, **case)
    st, finished, figures, preemptions = _run(which, N_TOP, **case)
    assert st.finished == st0.finished == 16 and st.total_tokens == st0.total_tokens
    assert sorted(finished) == sorted(plain)
    for item_id in plain:
        assert np.array_equal(plain[item_id], finished[item_id]), f"item {item_id}: tokens change with logprobs"
    if "half the pool" in name:
        assert preemptions > 0, "the case is there for the preempted rows"
    _judge(f"{name}, {which}", which, case, finished, figures)


@pytest.mark.parametrize("which", ["greedy", "top-p"])
def test_the_two_loops_agree_within_twice_the_bound(mli, dev, which):
    seq, pipe = CASES["PAGED, sequential"], CASES["PAGED, pipelined, half the pool"]
    _, fin_s, fig_s, _ = _run(which, N_TOP, **seq)
    _, fin_p, fig_p, _ = _run(which, N_TOP, **pipe)
    bounds = _judge(f"PAGED sequential (loops), {which}", which, seq, fin_s, fig_s)
    worst = 0.0
    for item_id, bound in bounds.items():
        assert np.array_equal(fin_s[item_id], fin_p[item_id])
        d = float(np.abs(fig_s[item_id][1].astype(np.float64) - fig_p[item_id][1]).max())
        worst = max(worst, d / bound)
        assert d <= 2 * bound, (item_id, d, bound)
    print(f"LOGPROBS engine loops, {which}: the loops differ by at most {worst:.3g} bounds")


def test_set_logprobs_refusals_and_an_engine_without_logprobs(mli, dev):
    import ctypes
    from min_llm_inference_amd import engine as eng
    model, items, _ = _workload("greedy")
    args = (SHAPE["B"], SHAPE["S"], SHAPE["D"], SHAPE["V"], model["emb_table"], model["pos_table"], model["wk"], model["wq"],
            model["wv"])
    for kind in (eng.CONTIGUOUS, eng.PAGED, eng.PAGED_GEMM, eng.PAGED_BF16, eng.PAGED_FP8):      # accepted on all five kinds
        e = eng.Engine(kind, *args, n_blocks=0 if kind == eng.CONTIGUOUS else FULL)
        try:
            for bad in (-1, 9):
                with pytest.raises(eng.MliError, match="n_top"):
                    e.set_logprobs(bad)
            e.set_logprobs(0)
            e.set_logprobs(8)
        finally:
            e.close()
    e = eng.Engine(eng.PAGED, *args, n_blocks=FULL, reference_length_reset_quirk=True)
    try:
        with pytest.raises(eng.MliError, match="quirk"):
            e.set_logprobs(2)
    finally:
        e.close()
    e = eng.Engine(eng.PAGED, *args, n_blocks=FULL, logprobs=0)                                  # n_top 0: token logprobs alone
    try:
        e.add_item(*items[0])
        with pytest.raises(eng.MliError, match="duplicate"):
            e.add_item(*items[0])
        with pytest.raises(eng.MliError, match="duplicate"):
            e.add_item(items[0][0], items[0][1], temperature=0.8, seed=3)
        e.set_pipelined(False)
        e.step()
        with pytest.raises(eng.MliError, match="started"):
            e.set_logprobs(2)
        e.run()
        n_prompt, lp, ids, tops = e.finished_logprobs()[items[0][0]]
        assert n_prompt == len(items[0][1]) and len(lp) == len(e.finished()[0][1]) - n_prompt and ids.shape == (len(lp), 0)
        assert np.isfinite(lp).all() and (lp <= 0).all()
    finally:
        e.close()
    e = eng.Engine(eng.PAGED, *args, n_blocks=FULL)                                              # never asked for logprobs
    try:
        e.add_item(*items[0])
        e.add_item(*items[0])                                                                    # duplicates stay legal here
        with pytest.raises(eng.MliError, match="twice"):                                         # but the figures are keyed by id
            e.set_logprobs(1)
        e.run()
        n = ctypes.c_int()
        assert mli.mli_engine_get_finished_logprobs(e._h, 0, ctypes.byref(n), None, 0, ctypes.byref(n), None, None, 0) == -1
    finally:
        e.close()
