"""What tests/test_shape_limits_gpu.py relies on, proved without a GPU ("the frontier"): the sparse builder of
tests/limit_cases.py writes the pages the dense builders write, bit for bit; its judge passes the fp32 oracle and fails three
wrong models of tests/test_accuracy_model_cpu.py by at least 4x the project's tolerance; its per-row truth is the dense
multi-head / window / sinks / grouped models'; the restated LDS sum of the equal-shares launcher gives the figures worked out
from the source; every row of the frontier table points at the line that holds its rule and names tests that exist; and
every refusal of the table is MLI_ERR_BAD_ARG through the C ABI before anything is launched (a launch would fail here)."""
import os
import re

import numpy as np
import pytest

import f64_model as fm
import gqa_model as gm
import heads_model as hm
import limit_cases as lc
from accuracy_cases import apply_family
from test_accuracy_model_cpu import mutant_last_token_dropped, mutant_merge_without_rescale, mutant_token_L_included

GAP = 4.0
# (seed, lengths, S, D, H, family / families per head)
SMALL = [(11, [0, 1, 15, 16, 17, 31, 47, 63, 0, 33], 64, 64, 1, "late_peak"),
         (12, [127, 0, 64, 65, 2, 16, 100], 128, 32, 1, "offset-"),
         (13, [255, 17, 0, 1, 240, 16, 32, 200], 256, 64, 2, ("early_peak", "peaked"))]


def _poisoned(case, pool):
    pool = pool.reshape(case.pool.shape).copy()
    pool[case.dead_page, case.dead_slot, 1:] = np.nan
    return pool


@pytest.mark.parametrize("seed,lengths,S,D,H,family", SMALL)
def test_sparse_builder_writes_what_the_dense_builder_writes(oracle, seed, lengths, S, D, H, family):
    live = [b for b, n in enumerate(lengths) if n]
    sparse = lc.SparseCase(seed, lengths, S, D, families={b: family for b in live}, H=H)
    base = lc.SparseCase(seed, lengths, S, D, H=H)            # the same values before the families
    kt, v = base.dense()
    c = {"q_output": base.q, "kt_cache": kt, "lengths": base.lengths}
    q, kt = apply_family(c, family) if H == 1 else _per_head(c, H, family)
    pool = np.zeros(base.pool.size, np.float32)
    oracle.clone_to_pages(pool, base.table_offsets(), np.zeros((len(lengths), S, D), np.float32), kt, v, base.lengths)
    assert (sparse.table == base.table).all() and (sparse.q[live] == q[live]).all()    # (an empty row's q is never read)
    a, b = _poisoned(sparse, sparse.pool), _poisoned(base, pool)
    assert a.tobytes() == b.tobytes(), "the pools differ"
    # ... and the table: pages for L + 1 slots, none shared, every other entry empty
    assert (sparse.row_pages == [0 if n == 0 else -(-min(n + 1, S) // 16) for n in lengths]).all()
    used = sparse.table[sparse.table >= 0]
    assert len(used) == len(set(used.tolist())) == sparse.n_pages
    assert np.isnan(a).sum() == len(sparse.dead_page) * 2 * D > 0 and not np.isnan(a[sparse.tok_page, sparse.tok_slot]).any()


def _per_head(c, H, families):
    q, kt = c["q_output"].copy(), c["kt_cache"].copy()
    for h, family in enumerate(families):
        sl = hm.head_slice(h, H, q.shape[1])
        sub = {"q_output": np.ascontiguousarray(q[:, sl]), "kt_cache": np.ascontiguousarray(kt[:, sl, :]), "lengths": c["lengths"]}
        q[:, sl], kt[:, sl, :] = apply_family(sub, family)
    return q, kt


def _worst(res):
    """{family: (worst kernel error, tolerance)}"""
    return {f: (max(e), fm.tolerance(np.asarray(o))) for f, (e, o) in res.items()}


def test_the_judge_passes_the_oracle_and_fails_three_wrong_models(oracle):
    lengths = [0, 1, 2, 17, 63, 64, 65, 255, 256, 257, 300, 511, 0, 400]
    case = lc.SparseCase(21, lengths, 512, 64)
    kt, v = case.dense()
    rows = list(range(case.B))
    oracle_out = np.zeros((case.B, case.D), np.float32)
    wrong = {"a": np.zeros((case.B, case.D)), "b": np.zeros((case.B, case.D)), "h": np.zeros((case.B, case.D))}
    for b in rows:
        n = lengths[b]
        if n == 0:
            continue
        K, V = case.rows(b)
        oracle_out[b] = lc.row_truth(oracle, case.q[b], K, V)[0][2][2][0]
        qb, Kd, Vd = case.q[b].astype(np.float64), kt[b].astype(np.float64), v[b].astype(np.float64)
        x = (qb @ Kd) / np.sqrt(case.D)
        wrong["a"][b] = mutant_last_token_dropped(qb, Kd, Vd, n, x)
        wrong["b"][b] = mutant_token_L_included(qb, Kd, Vd, n, x)
        wrong["h"][b] = mutant_merge_without_rescale(qb, Kd, Vd, n, x)
    worst, tol = _worst(lc.judge_rows(oracle, case, case.rows, oracle_out, rows))["flat"]
    assert worst <= tol < 1e-5, (worst, tol)
    assert not lc.whole_output_faults(case, oracle_out)
    for name, got in wrong.items():
        w, t = _worst(lc.judge_rows(oracle, case, case.rows, got, rows))["flat"]
        print(f"wrong model ({name}): {w:.3e} against tol {t:.3e}")
        assert w >= GAP * t, (name, w, t)
    # what every row owes: a sentinel, a NaN, an empty row that is not zero
    for b, value in ((3, lc.SENTINEL), (5, np.nan), (0, 1e-30)):
        bad = oracle_out.copy()
        bad[b, 7] = value
        assert lc.whole_output_faults(case, bad)
        if b == 0:
            assert _worst(lc.judge_rows(oracle, case, case.rows, bad, [0]))["flat"][0] == np.inf


@pytest.mark.parametrize("H,Hkv,W,K", [(2, 2, 0, 0), (2, 2, 17, 0), (2, 2, 16, 4), (2, 1, 0, 0), (4, 2, 33, 5), (1, 1, 1, 0)])
def test_row_truth_is_the_dense_models(oracle, H, Hkv, W, K):
    lengths = [0, 1, 16, 17, 18, 40, 63, 33, 21]
    S, D = 64, 128
    case = lc.SparseCase(31, lengths, S, D)
    kt, v = case.dense()
    model = gm.model_gqa(case.q, kt, v, case.lengths, H, Hkv, W, K)
    want_oracle = gm.oracle_gqa(oracle, case.q, kt, v, case.lengths, H, Hkv, W, K)
    for b, n in enumerate(lengths):
        if n == 0:
            continue
        K_, V_ = case.rows(b)
        for h, (cols, m, (_, _, o)) in enumerate(lc.row_truth(oracle, case.q[b], K_, V_, H, Hkv, W, K)):
            assert np.array_equal(m.o[0], model.o[b, cols]) and m.o_scale[0] == model.o_scale[b, h], (b, h)
            assert np.array_equal(o[0], want_oracle[b, cols]), (b, h)


@pytest.mark.parametrize("H,Hkv,W,K", [(2, 2, 0, 0), (2, 2, 17, 0), (2, 2, 16, 4), (2, 1, 0, 0), (4, 2, 33, 5), (4, 2, 24, 20)])
def test_row_truth_with_slopes_and_with_a_cap_is_the_dense_models(oracle, H, Hkv, W, K):
    """limit_cases.row_truth with `slopes` / `cap` against alibi_model / softcap_model on a dense case (alibi_model.slope_sets: standard, negative, mixed;
    caps 50, 5 and 1 on q scaled by scale_q): the float64 attention and its condition scale agree to 1e-12, and
    the float32 evaluation that sets row_truth's tolerance passes the dense model's own tolerance."""
    import alibi_model as am
    import softcap_model as sc
    lengths = [1, 16, 17, 18, 40, 63, 33, 21]
    S, D = 64, 128
    case = lc.SparseCase(32, lengths, S, D, H=H, Hkv=Hkv, families={4: ("offset-", "late_peak")[:Hkv], 5: "early_peak"})
    kt, v = case.dense()
    q_cap = sc.scale_q(case.q, kt, case.lengths, H, Hkv)
    forms = [("slopes", s, case.q) for s in am.slope_sets(H).values()] + [("cap", c, q_cap) for c in sc.CAPS]
    for kind, arg, q in forms:
        m_, kw = (am, dict(slopes=arg)) if kind == "slopes" else (sc, dict(cap=arg))
        model = (am.AlibiModel if kind == "slopes" else sc.SoftcapModel)(q, kt, v, case.lengths, H, Hkv, arg, W, K)
        tol = m_.tolerance(model, m_.eval_fp32(q, kt, v, case.lengths, H, Hkv, arg, W, K))
        for b in range(len(lengths)):
            K_, V_ = case.rows(b)
            for h, (cols, m, (_, _, o)) in enumerate(lc.row_truth(oracle, q[b], K_, V_, H, Hkv, W, K, **kw)):
                assert np.abs(m.o[0] - model.o[b, cols]).max() <= 1e-12 * max(1.0, np.abs(model.o[b, cols]).max()), (kind, arg, b, h)
                assert abs(m.o_scale[0] - model.o_scale[b, h]) <= 1e-12 * model.o_scale[b, h], (kind, arg, b, h)
                assert fm.attention_error(o, m)[0] <= tol, (kind, arg, b, h)


def test_restated_lds_sum_gives_the_figures_worked_out_from_the_source():
    assert lc.stream_lds_bytes(2048, 12288, 512, "f32", 256) == 73988      # 72.25 KiB
    assert lc.stream_lds_bytes(2048, 16384, 512, "f32", 256) == 82180      # 80.25 KiB
    for elem in ("f32", "bf16", "fp8"):     # 512 floats per wave partial in all three: the same sum
        assert lc.stream_maxseg(512, elem) == (4, 512)
        assert lc.stream_lds_bytes(2048, 12288, 512, elem, 256) == 73988
        # steps of 2048: 14336 (76.25 KiB) is the last accepted length, 12288 lies inside the branch too
        assert lc.stream_lds_frontier(2048, 512, elem, 256) == (14336, 16384)
    assert lc.stream_maxseg(1024, "bf16") == (2, 1024) and lc.stream_maxseg(1024, "fp8") == (2, 1024)
    assert lc.stream_lds_frontier(2048, 1024, "bf16", 256) == (14336, 16384)
    assert 64 * 1024 < lc.stream_lds_bytes(2048, 14336, 1024, "bf16", 256) <= 80 * 1024


def test_every_limit_names_its_line_and_a_test_on_each_side():
    """Each limit is referenced by at least one near and one far test id -- a parametrised case of the GPU file, by the tuple
    that must be in the list the test is parametrised by, or the refusals that name the limit -- so deleting a case, a tuple
    of ORDER_SHAPES / SHARES / ..., or a refusal leaves a limit without a test and fails here."""
    import test_shape_limits_gpu as gpu
    names = [l.name for l in lc.LIMITS]
    assert len(set(names)) == len(names)
    text = open(os.path.join(lc.ROOT, "tests", lc.GPU + ".py")).read()
    defined = set(re.findall(r"^def (test_\w+)\(", text, flags=re.M))
    refused = {}
    for entry, args, limit, ct in lc.REFUSALS:
        refused.setdefault(limit, []).append((entry, args))
    for l in lc.LIMITS:
        lc.rule_line(l)                                   # the rule's text stands on exactly one line of its file
        assert l.near_tests, f"{l.name}: no test on the near side"
        if l.far_outcome == lc.REFUSED:
            assert refused.get(l.name) and not l.far_tests, f"{l.name}: no refusal on the far side"
        else:
            assert l.far_tests or l.far == "-", f"{l.name}: no test on the far side"
        for function, listname, item in l.near_tests + l.far_tests:
            assert function in defined, f"{l.name}: {function} does not exist"
            assert f"def {function}(" in text
            if listname is not None:
                assert item in getattr(gpu, listname), f"{l.name}: {item} is not in {listname}"
                # ... and the function is parametrised by that list
                head = text[:text.index(f"def {function}(")].rsplit("\n\n\n", 1)[-1]
                assert listname in head, f"{l.name}: {function} is not parametrised by {listname}"
    assert set(refused) == {l.name for l in lc.LIMITS if l.far_outcome == lc.REFUSED}


def test_design_holds_the_table():
    design = open(os.path.join(lc.ROOT, "DESIGN.md")).read()
    for row in lc.markdown_rows():
        assert row[:-1] in design, f"DESIGN.md does not hold the row: {row[:120]} ..."


def test_the_triples_bound_never_refuses():
    """stream_triples_bound(W) > ceil(S / 64) is no reachable fall-back: over every value mli_tune accepts for the split (0 ..
    60 per cent, granules of 16 .. 256 pages) and every n_sequence from kStMinSequence on (checked to 2^20; the bound grows
    with W / piece, the slots with W / 4, and the smallest piece is 6 pages), a row's triples fit its slots."""
    for dyn in range(0, 61):
        for gran in (16, 17, 63, 64, 255, 256):
            for S in list(range(1024, 8192, 16)) + [1 << k for k in range(13, 21)]:
                assert lc.stream_triples_bound(S // 16, dyn, gran) <= -(-S // 64), (dyn, gran, S)
    assert lc.stream_triples_bound(32, 60, 16) > -(-32 * 16 // 64)      # at n_sequence 512 it would bite: kStMinSequence keeps W >= 64


def test_softmax_v_lds_does_not_grow_with_the_width():
    """launch_softmax_v_impl: items of at most 1024 tokens (chunk_tokens forced; 512 by the heuristic) and slices of at most two
    lane loads per wave, whatever the width: 4096 + 512 + 8192 bytes at the most"""
    worst = max(lc.softmax_v_lds_bytes(ct, D, vec) for ct in (64, 128, 256, 512, 1024) for vec in (1, 4)
                for D in (4, 64, 66, 512, 2048, 16384, 1 << 20) if D % vec == 0)
    assert worst == 4096 + 512 + 8192


@pytest.mark.parametrize("entry,args,limit,ct", lc.REFUSALS)
def test_refusals_without_a_gpu(mli, entry, args, limit, ct):
    """A workspace pointer that is not null and a size beyond any need: the refusal is the shape's, not the workspace's.  No
    pointer is dereferenced by a launcher; a launch, had the rule let the shape through, fails here and returns a HIP error.
    The newer entry points (prompt, ALiBi, soft-cap, rotary, sink logits) also refuse a null data pointer, so each of their rows runs twice:
    with null pointers, as on the device, and with every data pointer set to an address that is never followed -- then the
    pointer checks pass, and the answer shows that the shape rule stands ahead of them and of every launch."""
    from min_llm_inference_amd import ops
    assert mli.mli_launch_counts_reset() == 0
    try:
        assert mli.mli_tune(b"chunk_tokens", ct) == 0
        assert lc.call_refusal(mli, entry, args, workspace=4096) == lc.BAD_ARG
        assert lc.call_refusal(mli, entry, args, workspace=4096, data=4096) == lc.BAD_ARG, "refused by a pointer check, not the shape"
    finally:
        assert mli.mli_tune(b"chunk_tokens", 0) == 0
    for family in ("scan_equal_shares", "scan_chunked", "scan_heads_window", "scan_heads_alibi", "scan_heads_softcap", "scan_prompt",
                   "scan_prompt_softcap", "scan_heads_sink_logits", "scan_prompt_sink_logits", "gemm_f32_rows64", "gemm_bf16_widened", "gemm_f32_rope", "gemm_bf16_rope", "fill_flat",
                   "fill_per_row", "prefill_fused", "prefill_two_launch"):
        assert ops.launch_count(family) == 0, family
