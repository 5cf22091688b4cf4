"""Proves on the CPU that the comparison of tests/test_gqa_scan_gpu.py bites (tests/gqa_model.py): at every (shape, H, Hkv) of
the GPU test the fp32 oracle on the expanded operands passes against the float64 model on the expanded operands with its
own tolerance, and five wrong models of grouped-query attention fail the same comparer at the same tolerance by at least 4x
(the margin of tests/test_heads_model_cpu.py):
  K/V head h % Hkv, grouping ignored (head h reads block h), K grouped but V not, V grouped but K not, scale 1 / sqrt(Dkv).
Each of them changes the probabilities or the V columns of at least one query head in every family, so every assignment sees
them -- except where the wrong model IS the right one and no input can tell: with Hkv = 1, h % Hkv == h // g == 0 for every
head and Dkv == head_dim.  There the two are asserted to pass, so that the exception cannot hide a comparison that never bites.
Also: expand_kv against its definition, g = 1 as the identity, and the family construction (the heads of a group differ)."""
import functools

import numpy as np
import pytest

import gqa_model as gm
import heads_model as hm
from accuracy_cases import base_case, edge_lengths

GAP = 4.0
CASES = [(seed, B, S, D, H, Hkv, chunks) for seed, B, S, D, heads, _, chunks in gm.GQA_SHAPES for H, Hkv, _ in heads]


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, chunks):
    return base_case(seed, B, S, D, edge_lengths(seed, B, S, chunks))


@pytest.mark.parametrize("assignment", hm.ASSIGNMENTS)
@pytest.mark.parametrize("seed,B,S,D,H,Hkv,chunks", CASES)
def test_oracle_passes_and_wrong_models_fail(oracle, seed, B, S, D, H, Hkv, chunks, assignment):
    c = _base(seed, B, S, D, chunks)
    q, kt = gm.apply_gqa_families(c, H, Hkv, assignment)
    v, L = c["v_cache"], c["lengths"]
    fams = gm.head_families(assignment, H, Hkv)
    model = gm.model_gqa(q, kt, v, L, H, Hkv)
    o_or = gm.oracle_gqa(oracle, q, kt, v, L, H, Hkv)
    assert (o_or[L == 0] == 0).all() and (L == 0).any()
    gm.assert_within(gm.compare(o_or, o_or, model, fams, what="oracle"), "oracle")
    for name, fn in gm.WRONG_MODELS.items():
        res = gm.compare(fn(q, kt, v, L, H, Hkv), o_or, model, fams, what=name)
        ratio = max(worst / tol for _, worst, tol in res)
        if gm.wrong_is_the_right_model(name, H, Hkv):
            assert ratio <= 1.0, (name, ratio)
        else:
            assert ratio >= GAP, (name, assignment, ratio)


def test_every_group_size_is_covered():
    gs = {H // Hkv for _, _, _, _, heads, _, _ in gm.GQA_SHAPES for H, Hkv, _ in heads}
    assert {2, 3, 4, 8} <= gs
    assert any(Hkv == 1 for *_, heads, _, _ in gm.GQA_SHAPES for _, Hkv, _ in heads)
    for elem in ("f32", "bf16"):      # one lane load per row and two, in both page types
        epl = 4 if elem == "f32" else 8
        njs = {-(-(D // epl) // 64) for _, _, _, D, _, elems, _ in gm.GQA_SHAPES if elem in elems}
        assert njs == {1, 2}, (elem, njs)


def test_expand_kv():
    rng = np.random.default_rng(5)
    D, H = 192, 6
    a = rng.standard_normal((3, 7, D)).astype(np.float32)
    for Hkv in (1, 2, 3, 6):
        g, hd = H // Hkv, D // H
        x = gm.expand_kv(a, H, Hkv)
        assert x.shape == a.shape
        for h in range(H):
            assert np.array_equal(x[..., h * hd:(h + 1) * hd], a[..., (h // g) * hd:(h // g + 1) * hd])
        # the columns >= Dkv do not reach the result
        b = a.copy()
        b[..., Hkv * hd:] = np.nan
        assert np.array_equal(gm.expand_kv(b, H, Hkv), x)
        assert np.array_equal(gm.expand_kv(a.transpose(0, 2, 1), H, Hkv, axis=1), x.transpose(0, 2, 1))
    assert np.array_equal(gm.expand_kv(a, H, H), a)
    with pytest.raises(AssertionError):
        gm.expand_kv(a, H, 4)


def test_the_heads_of_a_group_differ_and_stay_in_their_family():
    seed, B, S, D = 302, 24, 256, 512
    c = _base(seed, B, S, D, (64, 256))
    H, Hkv = 8, 2
    g, hd = H // Hkv, D // H
    for assignment in hm.ASSIGNMENTS:
        q, kt = gm.apply_gqa_families(c, H, Hkv, assignment)
        assert np.array_equal(kt[:, Hkv * hd:, :], c["kt_cache"][:, Hkv * hd:, :]), "columns >= Dkv stay as generated"
        fams = gm.kv_families(assignment, Hkv)
        model = gm.model_gqa(q, kt, c["v_cache"], c["lengths"], H, Hkv)
        live = c["lengths"] > 16
        for j in range(Hkv):
            heads = [model.o[live][:, (j * g + i) * hd:(j * g + i + 1) * hd] for i in range(g)]
            for i in range(1, g):
                assert not np.allclose(heads[i], heads[0], rtol=1e-3, atol=0), (assignment, fams[j], i)
    # offsets: the heads of a group see their K/V head's shift scaled by their factor
    q, kt = gm.apply_gqa_families(c, H, Hkv, "offsets")
    b = int(np.argmax(c["lengths"]))
    x0 = q[b, :hd].astype(np.float64) @ kt[b, :hd, :4].astype(np.float64) / np.sqrt(hd)
    x1 = q[b, hd:2 * hd].astype(np.float64) @ kt[b, :hd, :4].astype(np.float64) / np.sqrt(hd)
    assert (x0 > 150).all() and np.allclose(x1, gm.FACTORS[1] * x0, rtol=1e-5)
