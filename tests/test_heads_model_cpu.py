"""Proves on the CPU that the comparison of tests/test_heads_scan_gpu.py bites (tests/heads_model.py): at every shape of
the GPU test the per-head fp32 oracle passes against the per-head float64 model with its own tolerance, and five wrong
models of multi-head attention fail the same comparer at the same tolerance by at least 4x.  Which assignment of score
families catches which fault is reasoned from the arithmetic and asserted:
  heads ignored, scale 1 / sqrt(emb_dim), heads interleaved as d % H, head h's probabilities on head h + 1's V
      change every probability of every head: every assignment sees them at every shape;
  a running maximum shared by the heads of a row
      is the same softmax on paper; it fails where a head's scores lie ~400 below its neighbour's (exp underflows, then
      0 / 0): the `offsets` and `mixed` assignments, never `flat`.
Also: the head-aware CPU engine reproduces engine_sim.CpuEngine at one head."""
import functools

import numpy as np
import pytest

import heads_model as hm
from accuracy_cases import base_case, edge_lengths
from engine_sim import make_items, make_model, run_cpu_engine

GAP = 4.0
CASES = [(seed, B, S, D, H, chunks) for seed, B, S, D, heads, _, chunks in hm.HEAD_SHAPES for H in heads]


@functools.lru_cache(maxsize=2)
def _base(seed, B, S, D, chunks):
    return base_case(seed, B, S, D, edge_lengths(seed, B, S, chunks))


@pytest.mark.parametrize("assignment", hm.ASSIGNMENTS)
@pytest.mark.parametrize("seed,B,S,D,H,chunks", CASES)
def test_oracle_passes_and_wrong_models_fail(oracle, seed, B, S, D, H, chunks, assignment):
    c = _base(seed, B, S, D, chunks)
    q, kt = hm.apply_head_families(c, H, assignment)
    v, L = c["v_cache"], c["lengths"]
    model = hm.HeadsModel(q, kt, v, L, H)
    o_or = hm.oracle_heads(oracle, q, kt, v, L, H)
    assert (o_or[L == 0] == 0).all() and (L == 0).any()
    hm.assert_within(hm.compare(o_or, o_or, model, assignment, what="oracle"), "oracle")
    for name, fn in hm.WRONG_MODELS.items():
        res = hm.compare(fn(q, kt, v, L, H), o_or, model, assignment, what=name)
        ratio = max(worst / tol for _, worst, tol in res)
        if name == "shared running maximum" and assignment == "flat":
            assert ratio <= 1.0, (name, ratio)      # the same softmax: what only neighbouring offsets can show
        else:
            assert ratio >= GAP, (name, assignment, ratio)


def test_offsets_puts_opposite_offsets_on_neighbouring_heads():
    for H in (2, 3, 4, 8):
        fams = hm.families_of("offsets", H)
        assert all({fams[h], fams[h + 1]} == {"offset+", "offset-"} for h in range(H - 1))
        assert len(set(hm.families_of("mixed", H))) == min(H, 6)


@pytest.mark.parametrize("bf16", [False, True])
def test_heads_cpu_engine_is_the_cpu_engine_at_one_head(oracle, bf16):
    B, S, D, V = 8, 64, 128, 1024
    model = make_model(77, V, S, D)
    items = make_items(78, 12, 3, 20)
    want, _ = run_cpu_engine(oracle, model, items, B, S, bf16=bf16)
    got, gap = hm.run_heads_cpu_engine(oracle, model, items, B, S, 1, bf16=bf16)
    assert sorted(got) == sorted(want) and np.isfinite(gap) and gap >= 0
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    four, _ = hm.run_heads_cpu_engine(oracle, model, items, B, S, 4, bf16=bf16)
    assert any(not np.array_equal(four[k], want[k]) for k in want), "four heads decode what one head decodes"
