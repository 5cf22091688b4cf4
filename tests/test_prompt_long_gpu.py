"""The causal multi-query prompt scan (mli_prompt_scan_paged, mli_prompt_scan_paged_softcap) at n_sequence 4096:
what tests/test_prompt_scan_gpu.py (n_sequence 128) and tests/test_softcap_prompt_gpu.py (256) cannot reach -- a wave that walks
up to 64 pages with its stride of four, an online-softmax state rescaled as often, a dropped run of about 190 pages between the
sinks and the window, a sink run that ends inside its second page, the window hand-off at W 4095 / 4096.
tests/test_prompt_long_cpu.py proves on the CPU that the comparison bites at these lengths.

Rows (prompt_model.long_case): a limit_cases.SparseCase of eight rows -- dense virtual rows [n_q, D, S] do not fit at S 4096 and
D 1024 -- laid into shuffled pages, NaN in the slots above every row's last scored position, a NaN page behind every table entry
beyond it; bf16 values are read back from the device.  Every query is judged on its own with limit_cases.row_truth on the first
t + 1 tokens of its row; q is scaled per position (prompt_model.query_vectors), so that swapped queries show.

Shapes: the eleven of prompt_model.SHAPES, one per kernel variant.  Score families: one head -- late_peak and early_peak, by row
(instead of one pass per family: the truth of a query costs O(t D) on the host); several heads -- the mixed assignment on the
K/V heads.  Forms (prompt_model.LONG_FORMS) and segments (prompt_model.long_segments, by the variant's mli_prompt_scan_tq) are
described there.

  tolerance   f64_model.tolerance (8 x) of the fp32 CPU oracle's own error on the same tokens, per score family
  out         rows of `out` that belong to no query (a hole between two segments, a tail) keep their sentinel
  cross-check every query within twice the bound of mli_decode_scan_paged_gqa on the virtual row of length t + 1
  counter     one "scan_prompt" launch (capped: "scan_prompt_softcap") and no decode scan; a second launch gives the same bits

The capped kernel: the four several-head shapes of test_softcap_prompt_gpu.SHAPES at S 4096, caps softcap_model.CAPS, q scaled
so that the largest attended score is half the largest cap (softcap_model.scale_q's rule, per query on the sparse rows), judged
with row_truth's cap: the float64 expression, tolerance from its float32 evaluation.  The capped truth costs two evaluations per
(query, cap), so the capped test runs the segments that reach the long paths (the last query at 4095, the block at 16 k - 1, the
max_count segment beside the single query, the continuation at 3000) and leaves the two mid-row blocks to the plain test.

The kernel with sink logits (mli_prompt_scan_paged_sink_logits): the six several-head shapes on the same segments, described at
test_prompt_scan_long_sink_logits; tests/test_sink_logits_limits_cpu.py proves on the CPU that its comparison bites."""
import functools

import numpy as np
import pytest
import torch

import limit_cases as lc
import prompt_model as pm
import softcap_model as sc
from gpu_util import host
from helpers import assert_equal
from test_shape_limits_gpu import Pages
from test_softcap_prompt_gpu import SHAPES as CAPPED_SHAPES

pytestmark = pytest.mark.gpu

S = pm.LONG_S
HOLE_AFTER, HOLE, TAIL = 3, 2, 1     # `out` rows of no query: HOLE rows after segment HOLE_AFTER, TAIL rows at the end
DECODE_FAMILIES = ("scan_chunked", "scan_heads_window", "scan_equal_shares", "scan_heads_softcap")
_TRUTH = {}


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@functools.lru_cache(maxsize=1)
def _case(seed, D, H, Hkv, tq, elem, dev):
    _TRUTH.clear()
    return Pages(pm.long_case(seed, D, H, Hkv, tq), elem, dev)


@pytest.fixture(scope="module", autouse=True)
def _release_memory():
    yield
    _case.cache_clear()
    _sunk_case.cache_clear()
    _TRUTH.clear()
    _SUNK_TRUTH.clear()
    torch.cuda.empty_cache()


def _layout(segs, dev):
    """(segment arrays on the device with max_count, the out row of every query, rows of no query, rows of out)"""
    counts = [cnt for _, _, cnt in segs]
    dense = np.concatenate([[0], np.cumsum(counts)[:-1]])
    offsets = dense + np.where(np.arange(len(segs)) > HOLE_AFTER, HOLE, 0)
    where = np.concatenate([np.arange(o, o + cnt) for o, cnt in zip(offsets, counts)])
    n_rows = sum(counts) + HOLE + TAIL
    nobody = np.setdiff1d(np.arange(n_rows), where)
    assert len(nobody) == HOLE + TAIL
    arrays = tuple(_t(np.asarray(a, np.int32), dev) for a in ([r for r, _, _ in segs], [f for _, f, _ in segs], counts, offsets))
    return arrays + (max(counts),), where, nobody, n_rows


def _launch(ops, x, q_dev, seg_arrays, n_rows, D, elem, H, Hkv, W, K, cap=None):
    out = torch.full((n_rows, D), lc.SENTINEL, device=q_dev.device)
    ops.prompt_scan_paged(q_dev, x.table, None, out, x.case.B, S, lc.ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K,
                          seg_arrays=seg_arrays, softcap=cap)
    return host(out).copy()


@pytest.mark.parametrize("W,K", pm.LONG_FORMS)
@pytest.mark.parametrize("seed,D,H,Hkv,elem", pm.SHAPES)
def test_prompt_scan_long(oracle, mli, dev, seed, D, H, Hkv, elem, W, K):
    from min_llm_inference_amd import ops
    tq = ops.prompt_scan_tq(D, H, lc.ELEM[elem])
    x = _case(seed, D, H, Hkv, tq, elem, dev)
    segs = pm.long_segments(tq, W)
    rows, pos = pm.queries(segs)
    assert pos.max() == S - 1 and max(n for _, _, n in segs) == pm.LONG_MAX_COUNT
    n = len(rows)
    seg_arrays, where, nobody, n_rows = _layout(segs, dev)
    what = f"S{S} D{D} H{H}/{Hkv} {elem} W{W} K{K} TQ{tq}"
    qv = pm.query_vectors(x.case.q, rows, pos)
    q_dev = torch.full((n_rows, D), float("nan"), device=dev)
    q_dev[_t(where, dev)] = _t(qv, dev)

    ops.reset_launch_counts()
    got_all = _launch(ops, x, q_dev, seg_arrays, n_rows, D, elem, H, Hkv, W, K)
    counts = {f: ops.launch_count(f) for f in ("scan_prompt", "scan_prompt_softcap") + DECODE_FAMILIES}
    assert counts == dict({f: 0 for f in counts}, scan_prompt=1), counts
    assert (got_all[nobody] == lc.SENTINEL).all(), f"{what}: an out row of no query was written"
    got = got_all[where]
    assert np.isfinite(got).all() and (got != lc.SENTINEL).any(axis=1).all(), what
    assert_equal(_launch(ops, x, q_dev, seg_arrays, n_rows, D, elem, H, Hkv, W, K), got_all, what=f"{what}: second launch")

    truth = pm.long_truth(oracle, x.case, x.values_of, qv, rows, pos, H, Hkv, W, K, cache=_TRUTH)
    res = pm.long_compare(got, truth, what=what)

    # the decode scan on the virtual rows: row i = the pages of rows[i] with length pos[i] + 1
    vt, vL = x.table[_t(rows, dev)].contiguous(), _t((pos + 1).astype(np.int32), dev)
    ref = torch.full((n, D), lc.SENTINEL, device=dev)
    ops.decode_scan_paged_gqa(_t(qv, dev), vt, vL, ref, H, Hkv, W, K, lc.ELEM[elem], S)
    ref = host(ref)
    assert np.isfinite(ref).all(), what
    d = pm.long_distance(got, ref, truth)
    for family, _, tol in res:
        print(f"PROMPT LONG {what} | {family}: {d[family]:.3e} from the decode scan on the virtual rows, twice the bound {2 * tol:.3e}")
        assert d[family] <= 2 * tol, (what, family, d[family], tol)
    pm.hm.assert_within(res, what)


def capped_segments(tq):
    """prompt_model.long_segments without the two mid-row blocks and the window-edge segments (the plain test has them)"""
    return pm.long_reaching_segments(tq)


SUNK_SHAPES = [s for s in pm.SHAPES if s[2] > 1]                    # the single-head kernels have no sink logit
SUNK_FORMS = [(0, 0), (1000, 20), (16, 0), (4095, 0)]
SUNK_RATIOS = []
_SUNK_TRUTH = {}


@functools.lru_cache(maxsize=1)
def _sunk_case(seed, D, H, Hkv, tq, elem, dev):
    _SUNK_TRUTH.clear()
    return Pages(pm.long_case(seed, D, H, Hkv, tq, families=pm.long_sink_families(Hkv)), elem, dev)


@pytest.mark.parametrize("W,K", SUNK_FORMS)
@pytest.mark.parametrize("seed,D,H,Hkv,elem", SUNK_SHAPES)
def test_prompt_scan_long_sink_logits(oracle, mli, dev, seed, D, H, Hkv, elem, W, K):
    """mli_prompt_scan_paged_sink_logits at n_sequence 4096 on the six several-head shapes of prompt_model.SHAPES: the segments the capped test keeps
    (the last query at 4095, the block at 16 k - 1, the max_count segment beside the single query, the continuation at 3000),
    rows in the families of prompt_model.long_sink_families -- a launch takes one logit per head for all of its queries --,
    logits per head from the judged queries at positions >= 1000 (limit_cases.learned_sparse over what the pages hold; the
    condition under which the comparison bites is asserted over those queries).  Every query is judged with
    row_truth(..., sink=z): the float64 expression, tolerance from its float32 evaluation.  Cross-check: within twice the bound
    of mli_decode_scan_paged_sink_logits on the virtual rows.  One "scan_prompt_sink_logits" launch and no other scan family;
    out rows of no query keep the sentinel; a second launch gives the same bits; all -inf gives the bits of the plain launch."""
    import sink_logits_model as sl
    from min_llm_inference_amd import ops
    tq = ops.prompt_scan_tq(D, H, lc.ELEM[elem])
    x = _sunk_case(seed, D, H, Hkv, tq, elem, dev)
    segs = capped_segments(tq)
    rows, pos = pm.queries(segs)
    assert pos.max() == S - 1 and max(n for _, _, n in segs) == pm.LONG_MAX_COUNT
    n = len(rows)
    seg_arrays, where, nobody, n_rows = _layout(segs, dev)
    what = f"S{S} D{D} H{H}/{Hkv} {elem} W{W} K{K} TQ{tq} sink logits"
    qv = pm.query_vectors(x.case.q, rows, pos)
    q_dev = torch.full((n_rows, D), float("nan"), device=dev)
    q_dev[_t(where, dev)] = _t(qv, dev)
    late = np.nonzero(pos >= 1000)[0]
    Wm, Km = (0, 0) if W >= S else (W, K)
    lse = lc.judged_lse(x.case, x.values_of, rows[late], H, Hkv, Wm, Km, q=qv[late], lengths=pos[late] + 1)
    z = lc.learned_sparse(lse)
    print(f"SINK_LOGITS PROMPT LONG {what}: logits {[round(float(t), 2) for t in z]}; the sink's share lies in {sl.SHARE_BAND} on "
          f"{lc.biting(lse, z, what):.2f} of the (query, head) pairs that set them")
    z_dev = _t(z, dev)

    def launch(logits):
        out = torch.full((n_rows, D), lc.SENTINEL, device=dev)
        ops.prompt_scan_paged(q_dev, x.table, None, out, x.case.B, S, lc.ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K,
                              seg_arrays=seg_arrays, sink_logits=logits)
        return host(out).copy()

    families = ("scan_prompt", "scan_prompt_softcap", "scan_prompt_sink_logits", "scan_heads_sink_logits") + DECODE_FAMILIES
    ops.reset_launch_counts()
    got_all = launch(z_dev)
    counts = {f: ops.launch_count(f) for f in families}
    assert counts == dict({f: 0 for f in counts}, scan_prompt_sink_logits=1), counts
    assert (got_all[nobody] == lc.SENTINEL).all(), f"{what}: an out row of no query was written"
    got = got_all[where]
    assert np.isfinite(got).all() and (got != lc.SENTINEL).any(axis=1).all(), what
    assert_equal(launch(z_dev), got_all, what=f"{what}: second launch")
    plain = _launch(ops, x, q_dev, seg_arrays, n_rows, D, elem, H, Hkv, W, K)
    assert_equal(launch(_t(sl.none(H), dev)), plain, what=f"{what}: all -inf against the plain long launch")
    assert np.abs(got - plain[where]).max() > 1e-3, f"{what}: the logits change nothing"

    truth = pm.long_truth(oracle, x.case, x.values_of, qv, rows, pos, H, Hkv, W, K, cache=_SUNK_TRUTH, sink=z)
    res = pm.long_compare(got, truth, what=what)
    SUNK_RATIOS.extend(worst / tol for _, worst, tol in res)
    print(f"SINK_LOGITS PROMPT LONG: worst got/tol over {len(SUNK_RATIOS)} comparisons so far {max(SUNK_RATIOS):.3f}")

    # the decode scan with the same logits on the virtual rows: row i = the pages of rows[i] with length pos[i] + 1
    vt, vL = x.table[_t(rows, dev)].contiguous(), _t((pos + 1).astype(np.int32), dev)
    ref = torch.full((n, D), lc.SENTINEL, device=dev)
    ops.decode_scan_paged_sink_logits(_t(qv, dev), vt, vL, ref, H, Hkv, W, K, z_dev, lc.ELEM[elem], S)
    ref = host(ref)
    assert np.isfinite(ref).all(), what
    d = pm.long_distance(got, ref, truth)
    for family, _, tol in res:
        print(f"PROMPT LONG {what} | {family}: {d[family]:.3e} from the decode scan on the virtual rows, twice the bound {2 * tol:.3e}")
        assert d[family] <= 2 * tol, (what, family, d[family], tol)
    pm.hm.assert_within(res, what)


def _scaled_q(x, qv, rows, pos, H, Hkv):
    """softcap_model.scale_q on the sparse rows: q scaled so that the largest |score| a query sees in its causal range is half
    the largest cap"""
    hd, g = x.case.D // H, H // Hkv
    top = 0.0
    held = {}
    for i in range(len(rows)):
        b, t = int(rows[i]), int(pos[i])
        if b not in held:
            held[b] = x.values_of(b)[0].astype(np.float64)
        for h in range(H):
            score = held[b][:t + 1, (h // g) * hd:(h // g + 1) * hd] @ qv[i, h * hd:(h + 1) * hd].astype(np.float64)
            top = max(top, float(np.abs(score).max()) / np.sqrt(hd))
    return (qv * np.float32(sc.CAPS[0] / 2 / top)).astype(np.float32)


@pytest.mark.parametrize("W,K", pm.LONG_FORMS)
@pytest.mark.parametrize("seed,B,S0,D,H,elem", CAPPED_SHAPES)
def test_capped_prompt_scan_long(oracle, mli, dev, seed, B, S0, D, H, elem, W, K):
    from min_llm_inference_amd import ops
    Hkv = 2
    tq = ops.prompt_scan_tq(D, H, lc.ELEM[elem])
    x = _case(seed, D, H, Hkv, tq, elem, dev)
    segs = capped_segments(tq)
    rows, pos = pm.queries(segs)
    assert pos.max() == S - 1 and max(n for _, _, n in segs) == pm.LONG_MAX_COUNT
    n = len(rows)
    seg_arrays, where, nobody, n_rows = _layout(segs, dev)
    if "q" not in _TRUTH:
        _TRUTH["q"] = _scaled_q(x, pm.query_vectors(x.case.q, rows, pos), rows, pos, H, Hkv)
    qv = _TRUTH["q"]
    q_dev = torch.full((n_rows, D), float("nan"), device=dev)
    q_dev[_t(where, dev)] = _t(qv, dev)
    vt, vL = x.table[_t(rows, dev)].contiguous(), _t((pos + 1).astype(np.int32), dev)
    plain = _launch(ops, x, q_dev, seg_arrays, n_rows, D, elem, H, Hkv, W, K)[where]
    results = []
    for cap in sc.CAPS:
        what = f"S{S} D{D} H{H}/{Hkv} {elem} W{W} K{K} TQ{tq} cap {cap:g}"
        ops.reset_launch_counts()
        got_all = _launch(ops, x, q_dev, seg_arrays, n_rows, D, elem, H, Hkv, W, K, cap=cap)
        counts = {f: ops.launch_count(f) for f in ("scan_prompt", "scan_prompt_softcap") + DECODE_FAMILIES}
        assert counts == dict({f: 0 for f in counts}, scan_prompt_softcap=1), counts
        assert (got_all[nobody] == lc.SENTINEL).all(), f"{what}: an out row of no query was written"
        got = got_all[where]
        assert np.isfinite(got).all() and (got != lc.SENTINEL).any(axis=1).all(), what
        assert_equal(_launch(ops, x, q_dev, seg_arrays, n_rows, D, elem, H, Hkv, W, K, cap=cap), got_all, what=f"{what}: second launch")
        truth = pm.long_truth(oracle, x.case, x.values_of, qv, rows, pos, H, Hkv, W, K, cap=cap, cache=_TRUTH)
        res = pm.long_compare(got, truth, what=what)
        if cap == sc.CAPS[1]:
            assert np.abs(got - plain).max() > 1e-3, f"{what}: the cap changes nothing"
        # the capped decode scan on the virtual rows, at every cap
        ref = torch.full((n, D), lc.SENTINEL, device=dev)
        ops.decode_scan_paged_softcap(_t(qv, dev), vt, vL, ref, H, Hkv, W, K, cap, lc.ELEM[elem], S)
        ref = host(ref)
        assert np.isfinite(ref).all(), what
        d = pm.long_distance(got, ref, truth)
        for family, _, tol in res:
            print(f"PROMPT LONG {what} | {family}: {d[family]:.3e} from the capped decode scan on the virtual rows, "
                  f"twice the bound {2 * tol:.3e}")
            assert d[family] <= 2 * tol, (what, family, d[family], tol)
        results += [(f"{family} cap {cap:g}", worst, tol) for family, worst, tol in res]
    pm.hm.assert_within(results, f"S{S} D{D} H{H}/{Hkv} {elem} W{W} K{K}")
