"""mli_score_tokens_logprobs against the float64 model of tests/logprobs_model.py with GIVEN tokens
(prompt_model.given_reference / compare_given): the rows of logprobs_model.families -- flat, peaked, +-200 offsets, exact ties
inside the top 8, -inf / +inf / NaN entries, all -inf (no finite logit), plain rows -- at n_vocab 1024 and 1000 (no multiple of
64), n_top 0, 3 and 8.

  targets     per row: the largest logit, the smallest, one in the middle, one whose logit is not finite where the row has one,
              and targets outside [0, n_vocab) (-1, n_vocab, 2^30): -inf for the token, the alternatives all the same
  figures     ids exactly the model's, logprobs within f64_model.tolerance of the float32 restatement's own error; the given
              token's logprob bit-equal to its entry in the list; two launches give the same bits
  bit equality with mli_sample_tokens_logprobs on greedy rows where the target is the greedy token"""
import numpy as np
import pytest
import torch

import logprobs_model as lm
import prompt_model as pm
from gpu_util import host
from test_sampling_gpu import _params, _t

pytestmark = pytest.mark.gpu


def _targets(x):
    """[n_sets, rows] given tokens"""
    V = x.shape[1]
    finite = np.where(np.isfinite(x), x, -np.inf)
    best = finite.argmax(axis=1)
    worst = np.where(np.isfinite(x), x, np.inf).argmin(axis=1)
    odd = np.asarray([int(np.nonzero(~np.isfinite(r))[0][-1]) if (~np.isfinite(r)).any() else V // 5 for r in x])
    odd2 = np.asarray([int(np.nonzero(~np.isfinite(r))[0][0]) if (~np.isfinite(r)).any() else V - 1 for r in x])
    out_of_range = np.resize(np.asarray([-1, V, 2 ** 30, -2 ** 31, V + 7]), len(x))
    return np.stack([best, worst, np.full(len(x), V // 2), odd, odd2, out_of_range]).astype(np.int32)


@pytest.mark.parametrize("n_top", [0, 3, 8])
@pytest.mark.parametrize("V", [1024, 1000])
def test_given_tokens_are_scored_as_the_model_scores_them(mli, dev, V, n_top):
    from min_llm_inference_amd import ops
    x, _ = lm.families(V)
    d_x = _t(np.array(x), dev)
    for given in _targets(x):
        got = [host(a) for a in ops.score_tokens_logprobs(d_x, _t(given, dev), n_top=n_top)]
        again = [host(a) for a in ops.score_tokens_logprobs(d_x, _t(given, dev), n_top=n_top)]
        err, tol, bad = pm.compare_given(got, x, given, n_top)
        print(f"SCORE V{V} n_top {n_top} targets {given.tolist()}: error {err:.3e} tolerance {tol:.3e}")
        assert not bad, bad
        assert err <= tol, (err, tol)
        for a, b in zip(got, again):
            assert a.tobytes() == b.tobytes(), "two launches differ"
        outside = (given < 0) | (given >= V)
        assert (got[0][outside] == -np.inf).all()
        if n_top and outside.any():
            assert (got[1][outside & np.isfinite(x).any(axis=1)] >= 0).any(), "alternatives of a row whose target is out of range"
    no_finite = ~np.isfinite(x).any(axis=1)
    assert no_finite.any()


@pytest.mark.parametrize("V", [1024, 1000])
def test_the_greedy_token_scores_with_the_bits_the_sampled_head_reports(mli, dev, V):
    from min_llm_inference_amd import ops
    x, _ = lm.families(V)
    B = len(x)
    d_x = _t(np.array(x), dev)
    lengths = _t(np.full(B, 5, np.int32), dev)                       # no empty row: every row emits
    params = _params(dev, np.zeros(B), np.zeros(B), np.ones(B), np.arange(B, dtype=np.int64))
    for n_top in (0, 3, 8):
        tokens, lp, ids, tops = [host(a) for a in ops.sample_tokens_logprobs(d_x, *params, lengths, n_top=n_top)]
        emits = tokens >= 0
        assert emits.sum() >= 6
        got = [host(a) for a in ops.score_tokens_logprobs(d_x, _t(tokens.astype(np.int32), dev), n_top=n_top)]
        assert got[0][emits].tobytes() == lp[emits].tobytes(), "token_logprob differs in bits"
        assert got[1][emits].tobytes() == ids[emits].tobytes() and got[2][emits].tobytes() == tops[emits].tobytes()


def test_no_rows_is_a_no_op_and_bad_arguments_are_refused_on_a_live_device(mli, dev):
    x = torch.zeros((2, 64), device=dev)
    t = torch.zeros(2, dtype=torch.int32, device=dev)
    lp = torch.full((2,), 7.0, device=dev)
    p = lambda a: a.data_ptr()
    assert mli.mli_score_tokens_logprobs(p(x), p(t), p(lp), None, None, 0, 64, 0, None) == 0
    torch.cuda.synchronize()
    assert (host(lp) == 7.0).all()
    assert mli.mli_score_tokens_logprobs(p(x), p(t), p(lp), None, None, 2, 64, 1, None) == -22
    assert mli.mli_score_tokens_logprobs(p(x), p(t), p(lp), None, None, 2, 64, 9, None) == -22
    assert mli.mli_score_tokens_logprobs(p(x), p(t), None, None, None, 2, 64, 0, None) == -22
    assert mli.mli_score_tokens_logprobs(p(x), p(t), p(lp), None, None, 2, 0, 0, None) == -22
