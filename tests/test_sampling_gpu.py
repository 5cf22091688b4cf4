"""GPU checks of the sampled decoder head against the numpy reference of its contract (sampling_ref.py):
the token pick on drawn logits, the distribution of the draws, bit-identity with the fused greedy head at T == 0, the
decoder bookkeeping with T > 0, run-to-run determinism, and the engines that decode with it."""
import numpy as np
import pytest
import torch

import sampling_ref as ref
from gpu_util import host
from helpers import assert_equal, bf16_bits, build_page_pool
from sampling_cases import check_against_reference as _check_against_reference, drawn_case as _drawn_case

pytestmark = pytest.mark.gpu

FP8 = 2


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _params(dev, T, K, P, seed):
    return (_t(np.asarray(T, np.float32), dev), _t(np.asarray(K, np.int32), dev), _t(np.asarray(P, np.float32), dev),
            _t(np.asarray(seed, np.int64), dev))


@pytest.mark.parametrize("V,B", [(1, 64), (3, 96), (1024, 512), (50257, 96), (131072 + 5, 32), (15 * 1024 + 1, 64)])
def test_sample_tokens_match_the_reference(mli, dev, V, B):
    from min_llm_inference_amd import ops
    rng = np.random.default_rng(7000 + V)
    x, T, K, P, seed, lengths = _drawn_case(rng, B, V)
    got = host(ops.sample_tokens(_t(x, dev), *_params(dev, T, K, P, seed), _t(lengths, dev)))
    _check_against_reference(x, T, K, P, seed, lengths, got, f"V={V}")
    assert (got[lengths == 0] == -1).all()
    greedy_rows = ~(T > 0) & (lengths > 0)
    assert all(got[b] == ref.greedy(x[b]) for b in np.nonzero(greedy_rows)[0])


def test_sample_tokens_are_run_to_run_deterministic(mli, dev):
    from min_llm_inference_amd import ops
    rng = np.random.default_rng(7101)
    x, T, K, P, seed, lengths = _drawn_case(rng, 256, 50257)
    args = (_t(x, dev), *_params(dev, T, K, P, seed), _t(lengths, dev))
    a = host(ops.sample_tokens(*args))
    b = host(ops.sample_tokens(*args))
    assert np.array_equal(a, b)


def _chi2(tokens, x, T, K, P):
    from scipy import stats
    keep, _ = ref.kept_set(x, T, K, P)
    assert keep[tokens].all(), "a token outside the kept set"
    z = (x / np.float32(T)).astype(np.float64)
    q = np.where(keep, np.exp(z - z[keep].max()), 0.0)
    q /= q.sum()
    obs = np.bincount(tokens, minlength=len(x))[keep]
    return stats.chisquare(obs, q[keep] * len(tokens)).pvalue


@pytest.mark.parametrize("K,P", [(0, 1.0), (12, 1.0), (0, 0.8), (15, 0.9)])
def test_draws_follow_softmax_over_the_kept_set(mli, dev, K, P):
    """One row with ~20 probable tokens, replicated: distinct seeds at one position, then one seed at distinct
    positions.  Fixed seeds make the p-values deterministic."""
    from min_llm_inference_amd import ops
    rng = np.random.default_rng(7200)
    V, N, T = 1024, 16384, 0.9
    x = np.full(V, -30.0, np.float32)
    probable = rng.choice(V, 20, replace=False)
    x[probable] = rng.uniform(-1.5, 1.5, 20).astype(np.float32)
    xs = np.broadcast_to(x, (N, V))
    for seed, lengths in ((np.arange(N, dtype=np.int64) * 7919 + 3, np.full(N, 17, np.int32)),
                          (np.full(N, 424242, np.int64), np.arange(1, N + 1, dtype=np.int32))):
        toks = host(ops.sample_tokens(_t(xs, dev), *_params(dev, np.full(N, T), np.full(N, K), np.full(N, P), seed),
                                      _t(lengths, dev)))
        p = _chi2(toks, x, T, K, P)
        print(f"K={K} P={P}: chi-square p = {p:.4f}")
        assert p >= 1e-3


def _decoder_inputs(rng, B, S, D, V):
    emb = (rng.standard_normal((V, D)) * 0.1).astype(np.float32)   # logits of spread ~1: a draw that is not degenerate
    wpe = rng.standard_normal((S, D)).astype(np.float32)
    att = rng.standard_normal((B, D)).astype(np.float32)
    lengths = rng.integers(1, S, B).astype(np.int32)
    lengths[0] = 0                      # empty row
    lengths[1] = S - 1                  # L + 1 == S: finishes, no next embedding
    att[5] = emb[1023] * 300            # row 5 lands on EOF, greedily and sampled
    return emb, wpe, att, lengths


def _pages(dev, pool, table, elem):
    if elem == 1:
        p = _t(bf16_bits(pool).view(np.int16), dev)
        return p, _t(np.where(table >= 0, p.data_ptr() + 2 * table, 0).astype(np.int64), dev)
    if elem == FP8:
        from min_llm_inference_amd import ops
        p = ops.f32_to_fp8(_t(pool, dev))
        return p, _t(np.where(table >= 0, p.data_ptr() + table, 0).astype(np.int64), dev)
    p = _t(pool, dev)
    return p, _t(np.where(table >= 0, p.data_ptr() + 4 * table, 0).astype(np.int64), dev)


@pytest.mark.parametrize("layout", ["contiguous", 0, 1, FP8])
def test_all_greedy_sampled_head_is_bit_identical_to_the_fused_head(mli, dev, layout):
    from min_llm_inference_amd import ops
    rng = np.random.default_rng(7300)
    B, S, D, V = 300, 128, 256, 1024
    emb, wpe, att, lengths = _decoder_inputs(rng, B, S, D, V)
    T = np.zeros(B, np.float32)
    K = rng.integers(0, 5, B).astype(np.int32)   # ignored at T == 0
    P = np.full(B, 0.5, np.float32)
    seed = rng.integers(0, 2 ** 40, B)
    d_att, d_emb, d_wpe = _t(att, dev), _t(emb, dev), _t(wpe, dev)
    if layout == "contiguous":
        inp = rng.standard_normal((B, S, D)).astype(np.float32)
        x1, l1, r1 = _t(inp, dev), _t(lengths, dev), torch.full((B,), 77, dtype=torch.int32, device=dev)
        x2, l2, r2 = _t(inp, dev), _t(lengths, dev), torch.full((B,), 77, dtype=torch.int32, device=dev)
        ops.decoder_fused(d_att, d_emb, d_wpe, x1, l1, r1)
        ops.decoder_sampled(d_att, d_emb, d_wpe, x2, l2, r2, *_params(dev, T, K, P, seed))
    else:
        pool, table = build_page_pool(rng, lengths, S, D)
        x1, t1 = _pages(dev, pool, table, layout)
        x2, t2 = _pages(dev, pool, table, layout)
        l1, l2 = _t(lengths, dev), _t(lengths, dev)
        r1 = torch.full((B, 2), 77, dtype=torch.int32, device=dev)
        r2 = r1.clone()
        ops.paged_decoder_fused(d_att, d_emb, d_wpe, t1, l1, r1, 1, layout)
        ops.paged_decoder_sampled(d_att, d_emb, d_wpe, t2, l2, r2, 1, layout, *_params(dev, T, K, P, seed))
    torch.cuda.synchronize()
    assert torch.equal(r1, r2), "tokens"
    assert torch.equal(l1, l2), "lengths"
    assert torch.equal(x1.view(torch.uint8), x2.view(torch.uint8)), "embeddings / pages"
    got = host(r2)
    assert got.reshape(B, -1)[0, -1] == -1 and got.reshape(B, -1)[5, -1] == 1023


def _fp8_round(a):
    from min_llm_inference_amd import ops
    return host(ops.f32_to_fp8(torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()))


@pytest.mark.parametrize("layout", ["contiguous", 0, 1, FP8])
def test_sampled_head_tokens_lengths_and_next_embedding(mli, dev, layout):
    """T > 0: the tokens are the reference's draw on the logits the head computed, and the bookkeeping is the greedy
    head's: lengths L + 1 (0 on EOF or L + 1 == S), next embedding emb[tok] + wpe[L] in the element type."""
    from min_llm_inference_amd import ops
    rng = np.random.default_rng(7400)
    B, S, D, V = 200, 64, 128, 1030
    emb, wpe, att, lengths = _decoder_inputs(rng, B, S, D, V)
    T = np.full(B, 1.1, np.float32)
    K, P = np.array([(0, 1.0), (40, 1.0), (40, 0.9)])[rng.integers(0, 3, B)].T
    K, P = K.astype(np.int32), P.astype(np.float32)
    seed = rng.integers(0, 2 ** 62, B)
    d_att, d_emb, d_wpe = _t(att, dev), _t(emb, dev), _t(wpe, dev)
    # the logits the head computes: the materialising greedy launcher runs the same GEMM into emb_score
    score = torch.zeros(B, V, device=dev)
    ops.launch_decoder(d_att, d_emb, score, d_wpe, _t(np.zeros((B, S, D), np.float32), dev), _t(lengths, dev),
                       torch.zeros(B, dtype=torch.int32, device=dev))
    logits = host(score)
    d_len = _t(lengths, dev)
    if layout == "contiguous":
        x = _t(np.zeros((B, S, D), np.float32), dev)
        res = torch.full((B,), 77, dtype=torch.int32, device=dev)
        ops.decoder_sampled(d_att, d_emb, d_wpe, x, d_len, res, *_params(dev, T, K, P, seed))
    else:
        pool = np.zeros((B * (S // 16) * 16 * 3 * D,), np.float32)
        table = (np.arange(B * (S // 16)) * 16 * 3 * D).reshape(B, S // 16).astype(np.int64)
        x, ptrs = _pages(dev, pool, table, layout)
        res = torch.full((B, 1), 77, dtype=torch.int32, device=dev)
        ops.paged_decoder_sampled(d_att, d_emb, d_wpe, ptrs, d_len, res, 0, layout, *_params(dev, T, K, P, seed))
    toks = host(res).reshape(B)
    _check_against_reference(logits, T, K, P, seed, lengths, toks, f"decoder head, {layout}")
    assert (toks != np.array([ref.greedy(r) for r in logits])).sum() > B // 4, "the draw is active"
    new_len = np.where((lengths + 1 >= S) | (toks == 1023), 0, lengths + 1)
    new_len[lengths == 0] = 0
    assert_equal(host(d_len), new_len.astype(np.int32), what="lengths")
    assert toks[0] == -1 and toks[5] == 1023 and new_len[1] == 0
    out = host(x.view(torch.uint8)).view(np.uint8)
    for b in range(B):
        L = int(lengths[b])
        wrote = L > 0 and L + 1 < S and toks[b] != 1023
        row = emb[toks[b]] + wpe[L] if wrote else np.zeros(D, np.float32)
        if layout == "contiguous":
            got = out.view(np.float32).reshape(B, S, D)[b, L] if L > 0 else None
            if got is not None:
                assert_equal(got, row, what=f"row {b}")
            continue
        off = int(table[b, L // 16]) + (L % 16) * 3 * D  # element offset of segment 0 at position L
        if layout == 0:
            assert_equal(out.view(np.float32)[off:off + D], row, what=f"row {b}")
        elif layout == 1:
            assert_equal(out.view(np.uint16)[off:off + D], bf16_bits(row).view(np.uint16), what=f"row {b}")
        else:
            assert_equal(out[off:off + D], _fp8_round(row).view(np.uint8), what=f"row {b}")


# ---- engines ---------------------------------------------------------------------------------------------------------

ENGINE_T, ENGINE_P = 0.8, 0.95


def _engine_run(kind, model, items, B, S, n_blocks=0, rounds=1, pipelined=False, graphs=False, sampled=None):
    """sampled: item id -> dict(temperature=..., top_k=..., top_p=..., seed=...); items not in it are queued plainly."""
    from min_llm_inference_amd import engine as eng
    D = model["wk"].shape[0]
    V = model["emb_table"].shape[0]
    e = eng.Engine(kind, B, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"], model["wv"],
                   n_blocks=n_blocks, n_forward_rounds=rounds)
    if kind != eng.CONTIGUOUS:
        e.set_pipelined(bool(pipelined))
    if graphs:
        e.use_private_stream()
        e.configure(step_graphs=True)
    for item_id, toks in items:
        e.add_item(item_id, toks, **(sampled or {}).get(item_id, {}))
    st = e.run()
    out = {i: t for i, t in e.finished()}
    e.close()
    assert st.finished == len(items)
    return out


def _engine_case():
    from engine_sim import make_items, make_model
    S, D, V = 128, 64, 1024
    model = make_model(7500, V, S, D)
    items = make_items(7501, 40, 1, 60)
    sampled = {i: dict(temperature=ENGINE_T, top_p=ENGINE_P, seed=1000003 * i + 17) for i, _ in items}
    return model, items, sampled, S


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for i in a:
        assert len(a[i]) == len(b[i]) and (a[i] == b[i]).all(), (what, i)


@pytest.mark.parametrize("kind_name", ["PAGED", "PAGED_GEMM", "PAGED_BF16", "PAGED_FP8"])
def test_sampled_engine_tokens_do_not_depend_on_scheduling(mli, dev, kind_name):
    from min_llm_inference_amd import engine as eng
    kind = getattr(eng, kind_name)
    model, items, sampled, S = _engine_case()
    ample = S // 16
    base = _engine_run(kind, model, items, 8, S, n_blocks=ample * 8, sampled=sampled)
    greedy = _engine_run(kind, model, items, 8, S, n_blocks=ample * 8)
    n_diff = sum(not (len(base[i]) == len(greedy[i]) and (base[i] == greedy[i]).all()) for i, _ in items)
    print(f"{kind_name}: {n_diff} of {len(items)} items differ from their greedy tokens")
    assert n_diff >= len(items) // 4, "the draw is active"
    for i, t in items:
        assert (base[i][:len(t)] == t).all() and (len(base[i]) == S or base[i][-1] == 1023)
    for what, kw in (("pipelined", dict(B=8, n_blocks=ample * 8, pipelined=True)),
                     ("4 rounds", dict(B=8, n_blocks=ample * 8, rounds=4)),
                     ("4 rounds pipelined", dict(B=8, n_blocks=ample * 8, rounds=4, pipelined=True)),
                     ("n_batch 48", dict(B=48, n_blocks=ample * 48)),
                     ("preemption", dict(B=48, n_blocks=4 * 48)),
                     ("preemption pipelined", dict(B=48, n_blocks=4 * 48, pipelined=True)),
                     ("step graphs", dict(B=8, n_blocks=ample * 8, graphs=True))):
        B = kw.pop("B")
        _assert_same(base, _engine_run(kind, model, items, B, S, sampled=sampled, **kw), f"{kind_name}: {what}")


def test_sampled_contiguous_engine(mli, dev):
    from min_llm_inference_amd import engine as eng
    model, items, sampled, S = _engine_case()
    base = _engine_run(eng.CONTIGUOUS, model, items, 8, S, sampled=sampled)
    _assert_same(base, _engine_run(eng.CONTIGUOUS, model, items, 48, S, sampled=sampled), "contiguous: n_batch 48")
    greedy = _engine_run(eng.CONTIGUOUS, model, items, 8, S)
    assert sum(not (len(base[i]) == len(greedy[i]) and (base[i] == greedy[i]).all()) for i, _ in items) >= len(items) // 4


def test_sampled_engine_seeds_and_mixed_batches(mli, dev):
    from min_llm_inference_amd import engine as eng
    model, items, sampled, S = _engine_case()
    a = _engine_run(eng.PAGED, model, items, 16, S, n_blocks=8 * 16, sampled=sampled)
    b = _engine_run(eng.PAGED, model, items, 16, S, n_blocks=8 * 16, sampled=sampled)
    _assert_same(a, b, "same seeds, two engines")
    other = {i: dict(p, seed=p["seed"] + 1) for i, p in sampled.items()}
    c = _engine_run(eng.PAGED, model, items, 16, S, n_blocks=8 * 16, sampled=other)
    assert sum(not (len(a[i]) == len(c[i]) and (a[i] == c[i]).all()) for i, _ in items) >= len(items) // 4
    # a mixed batch: the even items sampled, the odd ones queued plainly; the plain ones decode exactly as in a greedy
    # engine (a temperature-0 slot of the sampled head is the greedy head's token)
    mixed = {i: p for i, p in sampled.items() if i % 2 == 0}
    m = _engine_run(eng.PAGED, model, items, 16, S, n_blocks=8 * 16, sampled=mixed)
    g = _engine_run(eng.PAGED, model, items, 16, S, n_blocks=8 * 16)
    for i, _ in items:
        if i % 2:
            assert len(m[i]) == len(g[i]) and (m[i] == g[i]).all(), i
        else:
            assert len(m[i]) == len(a[i]) and (m[i] == a[i]).all(), i
    # temperature 0 through the sampled entry is greedy too
    zero = {i: dict(temperature=0.0, top_k=5, top_p=0.5, seed=9) for i, _ in items}
    _assert_same(g, _engine_run(eng.PAGED, model, items, 16, S, n_blocks=8 * 16, sampled=zero), "temperature 0")


def test_sampled_items_are_checked_and_the_head_is_fixed_at_the_first_step(mli, dev):
    import ctypes
    from min_llm_inference_amd import MliError
    from min_llm_inference_amd import engine as eng
    model, items, _, S = _engine_case()
    D, V = model["wk"].shape[0], model["emb_table"].shape[0]

    def make(**kw):
        return eng.Engine(eng.PAGED, 8, S, D, V, model["emb_table"], model["pos_table"], model["wk"], model["wq"],
                          model["wv"], n_blocks=64, **kw)

    e = make()
    toks = np.array([5, 6, 7], np.int32)
    ptr = toks.ctypes.data_as(ctypes.c_void_p)
    for T, K, P in ((-0.5, 0, 1.0), (float("nan"), 0, 1.0), (float("inf"), 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0),
                    (1.0, 0, 1.5), (1.0, 0, float("nan"))):
        assert e._lib.mli_engine_add_item_sampled(e._h, 1, ptr, 3, T, K, P, 0) == -1
        assert e._lib.mli_engine_last_error()
    e.add_item(1, toks, temperature=0.5, seed=3)
    with pytest.raises(MliError, match="duplicate"):
        e.add_item(1, toks, temperature=0.5, seed=4)
    e.close()
    q = make(reference_length_reset_quirk=True)
    with pytest.raises(MliError, match="quirk"):
        q.add_item(1, toks, temperature=0.5)
    q.close()
    # a greedy engine: after its first step a sampled item is refused, with a message, and the engine still finishes
    g = make()
    g.set_pipelined(False)
    for item_id, t in items[:12]:
        g.add_item(item_id, t)
    g.step()
    with pytest.raises(MliError, match="greedy head"):
        g.add_item(99, toks, temperature=0.8)
    g.add_item(100, toks, temperature=0.0, seed=5)   # temperature 0 is still welcome
    st = g.run()
    assert st.finished == 13 and st.waiting == 0
    g.close()
