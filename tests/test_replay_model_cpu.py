"""The engine replay audit (tests/replay_model.py) checked against itself, without a GPU:

  * the token streams of the four CPU engines (plain, heads, window, sinks; fp32, bf16 and fp8 modes; 1 and 4 heads) pass
    with deficit exactly 0 on every token;
  * a greedy generator built on the replay forward with one fault injected (replay_model.FAULTS) yields at least one token
    whose deficit is >= 4 tol, under the fp32 tolerance and under the bf16 tolerance with its rounding-flip envelope;
  * bookkeeping mutants and sampled mutants are rejected, and the sampled reference alone masks under 5 % of its draws.

Workload: n_batch 8, n_sequence 128, emb_dim 64, n_vocab 1024, 16 items with prompts of 3 .. 60 tokens, window 40 (three to
four pages, no multiple of 16), 4 sinks -- drawn freely, no seed search."""
import functools

import numpy as np
import pytest

import heads_model as hm
import replay_model as rm
import sampling_ref as sr
import sinks_model as sm
import window_model as wm
from engine_sim import make_items, make_model, run_cpu_engine

B, S, D, V, W, K = 8, 128, 64, 1024, 40, 4
N_ITEMS = 16
MODES = {"f32": False, "bf16": True, "fp8": "fp8"}


@functools.lru_cache(maxsize=1)
def _setup():
    return make_model(9101, V, S, D), make_items(9102, N_ITEMS, 3, 60)


CPU_CASES = [(engine, store, n_heads) for engine in ("plain", "heads", "window", "sinks") for store in ("f32", "bf16", "fp8")
             for n_heads in ((1,) if engine == "plain" else (4,) if engine == "heads" else (1, 4))]


@pytest.mark.parametrize("engine,store,n_heads", CPU_CASES)
def test_cpu_engine_streams_pass_with_deficit_zero(oracle, engine, store, n_heads):
    model, items = _setup()
    mode = MODES[store]
    if engine == "plain":
        tokens, _ = run_cpu_engine(oracle, model, items, B, S, bf16=mode)
        spec = rm.Spec(store)
    elif engine == "heads":
        tokens, _ = hm.run_heads_cpu_engine(oracle, model, items, B, S, n_heads, bf16=mode)
        spec = rm.Spec(store, n_heads)
    elif engine == "window":
        tokens, _ = wm.run_window_cpu_engine(oracle, model, items, B, S, n_heads, W, bf16=mode)
        spec = rm.Spec(store, n_heads, W)
    else:
        tokens, _ = sm.run_sinks_cpu_engine(oracle, model, items, B, S, n_heads, W, K, bf16=mode)
        spec = rm.Spec(store, n_heads, W, K)
    total = sum(len(tokens[i]) - len(t) for i, t in items)
    fig = rm.audit(model, items, tokens, spec, S, total_tokens=total, what=f"CPU {engine} engine")
    fig.assert_ok()
    assert fig.items == len(items) and fig.tokens == total
    assert fig.worst_deficit == 0.0 and fig.nonzero_deficits == 0, fig.line()


def test_the_generator_without_a_fault_passes_with_deficit_zero():
    model, items = _setup()
    for spec in (rm.Spec("f32", 4, W, K), rm.Spec("bf16", 4, W, K, flips=True), rm.Spec("fp8", 1, W, K, flips=True)):
        out = {i: rm.generate(model, t, spec, S, item_id=i) for i, t in items}
        fig = rm.audit(model, items, out, spec, S, what="generator, no fault")
        fig.assert_ok()
        assert fig.worst_deficit == 0.0
        if spec.flips:
            print(f"E_flip at R/2 {fig.e_flip_half:.3e}, at R {fig.e_flip:.3e}")
            assert fig.ambiguous > 0 and fig.e_flip > 0, "the workload has no rounding-ambiguous element: nothing is modelled"


@pytest.mark.parametrize("store", ["f32", "bf16"])
@pytest.mark.parametrize("fault", rm.FAULTS)
def test_a_wrong_generator_is_rejected_by_four_tolerances(fault, store):
    """The audit (the RIGHT model: 4 heads, window 40, 4 sinks) over the tokens of a generator with one fault.  bf16: the
    tolerance includes the rounding-flip envelope of the native bf16 MFMA."""
    model, items = _setup()
    spec = rm.Spec(store, 4, W, K, flips=store != "f32")
    out = {i: rm.generate(model, t, spec, S, fault=fault, item_id=i) for i, t in items}
    fig = rm.audit(model, items, out, spec, S, what=f"wrong generator: {fault}")
    assert not fig.bookkeeping, fig.bookkeeping
    print(f"REPLAY wrong generator [{store}] {fault}: factor reached {fig.worst_ratio:.1f} ({len(fig.failures)} of {fig.tokens} "
          f"tokens over tolerance)")
    assert fig.worst_ratio >= rm.MARGIN, fig.line()
    with pytest.raises(AssertionError):
        fig.assert_ok()


def _finished():
    model, items = _setup()
    spec = rm.Spec("f32")
    out = [(i, rm.generate(model, t, spec, S, item_id=i)) for i, t in items]
    # the bookkeeping judge reads no logits: two items are given an EOF by hand (these toy models rarely emit one)
    for n in (1, 5):
        i, t = out[n]
        p = len(items[n][1])
        out[n] = (i, np.append(t[:p + 2 + n], rm.EOF).astype(np.int32))
    assert not rm.bookkeeping(items, out, S, V, sum(len(t) - len(dict(items)[i]) for i, t in out))
    return items, out


def _ending(out, eof):
    for n, (i, t) in enumerate(out):
        if (t[-1] == rm.EOF) == eof and (eof or len(t) == S):
            return n
    raise AssertionError("the workload has no item that ends " + ("on EOF" if eof else "at n_sequence"))


def test_bookkeeping_mutants_are_rejected():
    items, out = _finished()
    total = sum(len(t) - len(dict(items)[i]) for i, t in out)

    def rejected(mutant, needle, total_tokens=None):
        bad = rm.bookkeeping(items, mutant, S, V, total_tokens)
        assert any(needle in b for b in bad), (needle, bad)

    n_eof, n_full = _ending(out, True), _ending(out, False)
    i, t = out[n_eof]
    rejected(out[:n_eof] + [(i, np.append(t, 5).astype(np.int32))] + out[n_eof + 1:], "the stream ends at")   # goes on after EOF
    rejected(out[:n_eof] + [(i, t[:-1])] + out[n_eof + 1:], "the stream ends at")                              # one short of EOF
    i, t = out[n_full]
    rejected(out[:n_full] + [(i, t[:-1])] + out[n_full + 1:], "the stream ends at")                            # one short of S
    i, t = out[0]
    changed = t.copy()
    changed[0] = (changed[0] + 1) % 1023
    rejected([(i, changed)] + out[1:], "prompt not intact")
    rejected(out[1:], "missing")
    rejected(out + [out[3]], "finished twice")
    outside = out[2][1].copy()
    outside[-2] = V
    rejected(out[:2] + [(out[2][0], outside)] + out[3:], "outside")
    rejected(out, "total_tokens", total_tokens=total + 1)
    model, _ = _setup()
    fig = rm.audit(model, items, out[1:], rm.Spec("f32"), S, what="an item missing")
    with pytest.raises(AssertionError, match="bookkeeping"):
        fig.assert_ok()


SAMPLED_SPECS = {"f32": rm.Spec("f32"), "bf16 exact, 4 heads, window": rm.Spec("bf16", 4, rm.SAMPLED_SHAPE["W"])}


def _sampled(spec, which, draw=None):
    """the workload of the sampled GPU tests (tests/test_engine_replay_gpu.py), decoded by the generator"""
    model, items, sampling = rm.sampled_workload(which)
    n_seq = rm.SAMPLED_SHAPE["S"]
    out = {i: rm.generate(model, t, spec, n_seq, params=sampling.get(i), item_id=i, draw=draw) for i, t in items}
    return model, items, out, sampling, n_seq


@pytest.mark.parametrize("params", sorted(rm.SAMPLED_PARAMS))
@pytest.mark.parametrize("spec_name", sorted(SAMPLED_SPECS))
def test_the_sampled_reference_alone_stays_under_the_masked_draw_cap(spec_name, params):
    spec = SAMPLED_SPECS[spec_name]
    model, items, out, sampling, n_seq = _sampled(spec, params)
    fig = rm.audit(model, items, out, spec, n_seq, sampling=sampling, what=f"sampled reference, {params}")
    fig.assert_ok()
    assert 0 < fig.draws < fig.tokens and fig.masked_share() <= rm.MASK_CAP, fig.line()
    assert fig.worst_deficit == 0.0, "the greedy half"
    greedy = {i: rm.generate(model, t, spec, n_seq, item_id=i) for i, t in items}
    assert all((greedy[i] != out[i]).any() if len(greedy[i]) == len(out[i]) else True for i in sampling)


MUTANTS = {
    "position counter off by one": lambda x, T, Kk, P, seed, L: sr.sample_row(x, T, Kk, P, seed, L + 1),
    "seed of another item": lambda x, T, Kk, P, seed, L: sr.sample_row(x, T, Kk, P, seed + 1, L),
    "temperature ignored": lambda x, T, Kk, P, seed, L: sr.greedy(x),
    "top-k ignored": lambda x, T, Kk, P, seed, L: sr.sample_row(x, T, 0, P, seed, L),
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_sampled_mutants_fail_on_well_posed_draws(mutant):
    spec = SAMPLED_SPECS["f32"]
    model, items, out, sampling, n_seq = _sampled(spec, "top-k", draw=MUTANTS[mutant])
    fig = rm.audit(model, items, out, spec, n_seq, sampling=sampling, what=f"sampled mutant: {mutant}")
    assert not fig.bookkeeping
    wrong = [f for f in fig.failures if "the reference draws" in f]
    print(f"REPLAY sampled mutant {mutant}: {len(wrong)} of {fig.draws - fig.masked_draws} well-posed draws rejected")
    assert wrong, fig.line()
    assert fig.masked_share() <= rm.MASK_CAP


def test_a_sampled_item_of_a_kind_with_rounding_flips_gets_the_bookkeeping_judge_alone():
    spec = rm.Spec("bf16", 4, W, flips=True)
    model, items, out, sampling, n_seq = _sampled(spec, "top-k")
    fig = rm.audit(model, items, out, spec, n_seq, sampling=sampling, what="sampled, native bf16")
    fig.assert_ok()
    assert fig.draws == 0 and fig.tokens > 0
    changed = dict(out)
    i = sorted(sampling)[0]
    changed[i] = np.append(out[i][:-1], (out[i][-1] + 1) % 1023).astype(np.int32)   # a wrong draw: not judged on this kind
    rm.audit(model, items, changed, spec, n_seq, sampling=sampling, what="sampled, native bf16, one draw changed").assert_ok()


def test_the_report_holds_the_figures_of_every_audited_case():
    model, items = _setup()
    spec = rm.Spec("f32")
    out = {i: rm.generate(model, t, spec, S, item_id=i) for i, t in items}
    fig = rm.audit(model, items, out, spec, S, what="report")
    row = rm.REPORT[fig.what]
    assert {"items", "tokens", "nonzero_deficits", "worst_deficit", "tol", "e32", "e_flip_half", "e_flip", "masked_draws"} <= set(row)
