"""GPU checks of the log-probability heads against the float64 model of tests/logprobs_model.py.

mli_sample_tokens_logprobs on the 8 rows of logprobs_model.families -- flat, peaked, +-200 offsets, exact ties inside the top
8, -inf / +inf / NaN entries, all -inf, an empty row, a plain row -- at n_vocab 1000 (no multiple of the thread count or of
4), 1024, 15 * 1024 + 4 (the first size past the LDS staging: every pass re-reads the row from L2) and 5 (fewer candidates
than n_top), n_top 0, 1, 3 and 8, greedy and T = 0.8 with top-k and with top-p:

  tokens         bit-identical to mli_sample_tokens on the same inputs
  top_ids        exactly the model's: (logit descending, index ascending) over the finite logits
  logprobs       within f64_model.tolerance(e) of the model, e = the float32 restatement's own error on the same logits in log
                 units (never a kernel's figure); padded entries and no-token rows as specified; the token's logprob bit-equal
                 to its entry in the list; two launches give the same bits

and the decoder forms: token, length and next embedding of the plain sampled heads, the figures those of the token pick on
the same logits, with n_decoder_results = 2 and i_decoder = 1 (the strides)."""
import functools

import numpy as np
import pytest
import torch

import logprobs_model as lm
from gpu_util import host
from helpers import build_page_pool
from test_sampling_gpu import FP8, _decoder_inputs, _pages, _params, _t

pytestmark = pytest.mark.gpu

SIZES = [1000, 1024, 15 * 1024 + 4, 5]
PARAMS = {"greedy": (0.0, 0, 1.0), "top-k": (0.8, 40, 1.0), "top-p": (0.8, 0, 0.95)}


@functools.lru_cache(maxsize=None)
def _case(V):
    x, lengths = lm.families(V)
    x.setflags(write=False)
    return x, lengths, lm.tolerance(x)


def _run(dev, x, lengths, which, n_top):
    from min_llm_inference_amd import ops
    B = len(x)
    T, K, P = PARAMS[which]
    params = _params(dev, np.full(B, T), np.full(B, K), np.full(B, P), np.arange(B, dtype=np.int64) * 7919 + 11)
    d_x, d_len = _t(np.array(x), dev), _t(lengths, dev)             # the shared case stays read-only: a copy travels
    plain = host(ops.sample_tokens(d_x, *params, d_len))
    got = [host(a) for a in ops.sample_tokens_logprobs(d_x, *params, d_len, n_top=n_top)]
    again = [host(a) for a in ops.sample_tokens_logprobs(d_x, *params, d_len, n_top=n_top)]
    return plain, got, again


@pytest.mark.parametrize("which", sorted(PARAMS))
@pytest.mark.parametrize("n_top", [0, 1, 3, 8])
@pytest.mark.parametrize("V", SIZES)
def test_token_logprobs_and_alternatives_match_the_model(mli, dev, V, n_top, which):
    x, lengths, tol = _case(V)
    plain, (tokens, lp, ids, tops), again = _run(dev, x, lengths, which, n_top)
    assert tokens.tobytes() == plain.tobytes(), "tokens differ from mli_sample_tokens"
    assert ids.shape == (8, n_top) and tops.shape == (8, n_top)
    err, tol2, bad = lm.compare((lp, ids, tops), x, tokens, n_top)
    print(f"LOGPROBS V {V} n_top {n_top} {which}: worst error {err:.3e} tol {tol:.3e}")
    assert tol2 == tol and not bad and err <= tol, (err, tol, bad)
    for a, b in zip((tokens, lp, ids, tops), again):
        assert a.tobytes() == b.tobytes(), "two launches differ"
    # the rows that emit nothing: all -inf (token -1) and empty (length 0)
    for b in (5, 6):
        assert tokens[b] == -1 and lp[b] == -np.inf and (ids[b] == -1).all() and (tops[b] == -np.inf).all()
    if which == "greedy":
        assert np.isnan(lp[4])                                     # the greedy pick takes the +inf entry: NaN, as specified
    else:
        assert np.isfinite(lp[4])
    if n_top == 8 and V == 5:
        assert (ids[0] == [0, 1, 2, 3, 4, -1, -1, -1]).all() and (tops[0, 5:] == -np.inf).all()
        np.testing.assert_allclose(tops[0, :5], -np.log(5.0), atol=tol)
    if n_top >= 3 and V >= 1000:
        assert ids[3, :3].tolist() == [0, V // 2, V - 1]           # three equal leaders, by index


@pytest.mark.parametrize("layout", ["contiguous", 0, 1, FP8])
def test_decoder_forms_keep_the_plain_heads_results_and_stride_the_figures(mli, dev, layout):
    from min_llm_inference_amd import ops
    rng = np.random.default_rng(7600)
    B, S, D, V, n_top = 24, 64, 128, 1030, 3
    emb, wpe, att, lengths = _decoder_inputs(rng, B, S, D, V)
    T = np.where(np.arange(B) % 2, 0.8, 0.0).astype(np.float32)
    K, P = np.full(B, 40, np.int32), np.full(B, 0.95, np.float32)
    seed = rng.integers(0, 2 ** 62, B)
    d_att, d_emb, d_wpe = _t(att, dev), _t(emb, dev), _t(wpe, dev)
    score = torch.zeros(B, V, device=dev)                           # the logits the heads compute (the same GEMM)
    ops.launch_decoder(d_att, d_emb, score, d_wpe, _t(np.zeros((B, S, D), np.float32), dev), _t(lengths, dev),
                       torch.zeros(B, dtype=torch.int32, device=dev))
    params = _params(dev, T, K, P, seed)
    r2 = torch.full((B, 2), 77, dtype=torch.int32, device=dev)
    l1, l2 = _t(lengths, dev), _t(lengths, dev)
    if layout == "contiguous":
        inp = rng.standard_normal((B, S, D)).astype(np.float32)
        x1, x2 = _t(inp, dev), _t(inp, dev)
        r1 = torch.full((B,), 77, dtype=torch.int32, device=dev)
        ops.decoder_sampled(d_att, d_emb, d_wpe, x1, l1, r1, *params)
        lp, ids, tops = ops.decoder_sampled_logprobs(d_att, d_emb, d_wpe, x2, l2, r2, 1, *params, n_top=n_top)
    else:
        pool, table = build_page_pool(rng, lengths, S, D)
        x1, t1 = _pages(dev, pool, table, layout)
        x2, t2 = _pages(dev, pool, table, layout)
        r1 = torch.full((B, 2), 77, dtype=torch.int32, device=dev)
        ops.paged_decoder_sampled(d_att, d_emb, d_wpe, t1, l1, r1, 1, layout, *params)
        lp, ids, tops = ops.paged_decoder_sampled_logprobs(d_att, d_emb, d_wpe, t2, l2, r2, 1, layout, *params, n_top=n_top)
    torch.cuda.synchronize()
    assert torch.equal(r1.reshape(B, -1)[:, -1], r2[:, 1]) and (r2[:, 0] == 77).all(), "tokens"
    assert torch.equal(l1, l2), "lengths"
    assert torch.equal(x1.view(torch.uint8), x2.view(torch.uint8)), "embeddings / pages"
    # the figures are those of the token pick on the same logits and positions, in column 1
    tok, w_lp, w_ids, w_tops = ops.sample_tokens_logprobs(score, *params, _t(lengths, dev), n_top=n_top)
    assert torch.equal(tok, r2[:, 1])
    for got, want in ((lp, w_lp), (ids, w_ids), (tops, w_tops)):
        assert host(got[:, 1].contiguous()).tobytes() == host(want).tobytes()
    err, tol, bad = lm.compare((host(w_lp), host(w_ids), host(w_tops)), host(score), host(tok), n_top)
    print(f"LOGPROBS decoder head, {layout}: worst error {err:.3e} tol {tol:.3e}")
    assert not bad and err <= tol, (err, tol, bad)
    assert host(tok)[0] == -1 and host(lp)[0, 1] == -np.inf and (host(ids)[0, 1] == -1).all()
