"""The kernels at the last shape their launchers accept, and on the far side of every silent fallback ("the
frontier").  One test stands on each side of every row of limit_cases.LIMITS; tests/test_shape_limits_cpu.py holds the table
to the code and proves the builder and the judge.

Judge: limit_cases.judge_rows -- per (row, head) condition-scaled error against the float64 model, tolerance
max(8 x E_oracle, 16 x 2^-24) from the fp32 CPU oracle on the same tokens, per score family.  Besides the numbers every launch
owes: no sentinel and nothing non-finite in ANY row, exact zeros for rows of length 0, the arrival counters and the ticket
zero afterwards, and the same bits from a second launch.  Which kernel ran is read from mli_launch_count.

A far-side shape runs here only where the launcher's own rule refuses or reroutes it before any launch (read in the code,
and for the refusals run without a GPU first, tests/test_shape_limits_cpu.py).  The workspace is the tests' own, allocated
uninitialised with the counter region zeroed once.  Knobs are set per test and restored."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import f64_model as fm
import limit_cases as lc
import prompt_model as pm
import softcap_model as sc
import stream_model as sm
from accuracy_cases import poison_contiguous
from accuracy_gpu import Checker
from gpu_util import host
from helpers import assert_equal, fp8_decode

pytestmark = pytest.mark.gpu

SCAN_FAMILIES = ("scan_equal_shares", "scan_chunked", "scan_rows_ordered", "scan_rows_grid_order", "scan_heads_window",
                 "scan_heads_alibi", "scan_heads_softcap", "scan_prompt", "scan_prompt_softcap", "scan_heads_sink_logits",
                 "scan_prompt_sink_logits")
# what a refusal must not have launched either: the projections and fills behind the prompt and rotary entry points
OTHER_FAMILIES = ("gemm_f32_rows64", "gemm_bf16_widened", "gemm_f32_rope", "gemm_bf16_rope", "fill_flat", "fill_per_row",
                  "prefill_fused", "prefill_two_launch")
CAP = 5.0
_WS = {}
SINK_RATIOS = []      # got / tol of every sink-logit comparison of this module, reported at its end


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.fixture(scope="module", autouse=True)
def _release_memory():
    yield
    if SINK_RATIOS:
        print(f"SINK_LOGITS limits: worst got/tol over {len(SINK_RATIOS)} comparisons {max(SINK_RATIOS):.3f}")
    SINK_RATIOS.clear()
    _WS.clear()
    _pages.cache_clear()
    for f in (_family_case, _scaled_q, _x_pages, _hand_off_case, _rows_case, _longest_case, _order_case, _shares_case, _heads_case, _merge_case, _offsets_case, _wide_case, _window_case, _lds_case):
        f.cache_clear()
    torch.cuda.empty_cache()


def _workspace(mli, dev, B, S, D, H=1):
    """(buffer, bytes needed): one uninitialised buffer, grown on demand, its counter region zeroed when it is made"""
    need = int(mli.mli_attention_workspace_bytes(B, S, D) if H == 1 else mli.mli_attention_heads_workspace_bytes(B, S, D, H))
    assert need > lc.COUNTER_BYTES
    ws = _WS.get("ws")
    if ws is None or ws.numel() < need:
        torch.cuda.synchronize()
        _WS.pop("ws", None)
        ws = None
        torch.cuda.empty_cache()
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        ws[:lc.COUNTER_BYTES] = 0
        _WS["ws"] = ws
    return ws, need


def _counters_are_zero(ws, what):
    assert not host(ws[:lc.COUNTER_BYTES]).any(), f"{what}: the arrival counters and the ticket are zero afterwards"


class Pages:
    """A SparseCase on the device in one page type: pool converted on the device, NaN in the dead slots of owned pages, a NaN
    page behind every other table entry; values_of(b) reads back what the row's pages hold."""

    def __init__(self, case, elem, dev):
        from min_llm_inference_amd import ops
        self.case, self.elem, self.dev = case, elem, dev
        pool = _t(case.pool, dev)
        nan = float("nan")
        if elem == "bf16":
            pool = pool.to(torch.bfloat16)
        elif elem == "fp8":
            assert ops.has_fp8()
            pool = ops.f32_to_fp8(pool)
            nan = 0x7F
            self.lut = _t(fp8_decode(np.arange(256, dtype=np.uint8)), dev)
        if len(case.dead_page):
            pool[_t(case.dead_page, dev), _t(case.dead_slot, dev), 1:] = nan
        self.pool = pool
        self.nan_page = torch.full((16 * 3 * case.D,), nan, dtype=pool.dtype, device=dev)
        page_bytes = 16 * 3 * case.D * lc.ESIZE[elem]
        self.table = _t(np.where(case.table >= 0, pool.data_ptr() + case.table * page_bytes, self.nan_page.data_ptr()), dev)
        self.q, self.L = _t(case.q, dev), _t(case.lengths, dev)
        self._pg, self._sl = _t(case.tok_page, dev), _t(case.tok_slot, dev)

    def values_of(self, b):
        lo, hi = int(self.case.start[b]), int(self.case.start[b + 1])
        kv = self.pool[self._pg[lo:hi], self._sl[lo:hi], 1:]
        kv = self.lut[kv.long()] if self.elem == "fp8" else kv.float()
        kv = kv.cpu().numpy()
        return kv[:, 0], kv[:, 1]


@functools.lru_cache(maxsize=1)
def _pages(case, elem, dev):
    return Pages(case, elem, dev)


def _tune(mli, **knobs):
    for k, v in knobs.items():
        assert mli.mli_tune(k.encode(), v) == 0, k


DEFAULTS = dict(chunk_tokens=0, scan_stream=1, scan_stream_min_tokens=1 << 21, scan_row_order=1)


def _call(mli, dev, x, entry, extra, elem, out, qkt=None, phases=7, H=1, q=None):
    """one launch through the C ABI; returns the status.  alibi: extra = (H, Hkv, W, K, slopes on the device); softcap: extra =
    (H, Hkv, W, K, cap); q: the queries where they are not the case's (limit_cases.scaled_q)"""
    c = x.case
    q = x.q if q is None else q
    ws, need = _workspace(mli, dev, c.B, c.S, c.D, H)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(0 if t is None else t.data_ptr())
    if entry == "scan":
        return mli.mli_decode_scan_paged(p(q), p(x.table), p(x.L), p(qkt), p(out), c.B, c.S, c.D, lc.ELEM[elem], phases, p(ws), need, st)
    if entry in ("alibi", "sink_logits"):       # extra = (H, Hkv, W, K, the slopes / the logits on the device)
        fn = mli.mli_decode_scan_paged_alibi if entry == "alibi" else mli.mli_decode_scan_paged_sink_logits
        return fn(p(q), p(x.table), p(x.L), p(out), c.B, c.S, c.D, *extra[:4], p(extra[4]), lc.ELEM[elem], p(ws), need, st)
    name = {"heads": "mli_decode_scan_paged_heads", "window": "mli_decode_scan_paged_window", "sinks": "mli_decode_scan_paged_sinks",
            "gqa": "mli_decode_scan_paged_gqa", "softcap": "mli_decode_scan_paged_softcap"}[entry]
    return getattr(mli, name)(p(q), p(x.table), p(x.L), p(out), c.B, c.S, c.D, *extra, lc.ELEM[elem], p(ws), need, st)


def _mask(S, W, K):
    """the (window, n_sink) the kernels mask by: lean_scan_kind's hand-offs give the plain mask"""
    if W <= 0 or W >= S:
        return 0, 0
    return (0, 0) if K + W >= S else (W, K)


def _learned(x, rows, H, Hkv, W, K, what):
    """(logits float32 [H], log-sum-exp of the judged pairs): limit_cases.learned_sparse from what the pages hold, with the
    condition under which the comparison bites (limit_cases.biting) asserted on the device's rounded values"""
    import sink_logits_model as sl
    lse = lc.judged_lse(x.case, x.values_of, rows, H, Hkv, *_mask(x.case.S, W, K))
    z = lc.learned_sparse(lse)
    f = lc.biting(lse, z, what)
    print(f"SINK_LOGITS {what}: logits {[round(float(t), 2) for t in z]}; the sink's share lies in {sl.SHARE_BAND} on {f:.2f} of the judged pairs")
    return z, lse


def _biased(entry, case, H, Hkv, W, K, dev, x=None, rows=None):
    """(arguments behind emb_dim, q on the device or None, the judge's keywords, the launch counter) of an ALiBi call with the
    slopes of mli_alibi_slopes, a soft-capped call at cap 5 with q scaled so that the largest score is 25 (scale_q's rule), or
    a call with sink logits learned from the judged `rows` of the pages `x` (_learned)"""
    from min_llm_inference_amd import ops
    if entry == "sink_logits":
        z, _ = _learned(x, rows, H, Hkv, W, K, f"sink_logits H {H}/{Hkv} W {W} K {K} {x.elem}")
        return (H, Hkv, W, K, _t(z, dev)), None, dict(sink=z), "scan_heads_sink_logits"
    if entry == "alibi":
        slopes = ops.alibi_slopes(H)
        return (H, Hkv, W, K, _t(slopes, dev)), None, dict(slopes=slopes), "scan_heads_alibi"
    q = _scaled_q(case, H, Hkv)
    return (H, Hkv, W, K, CAP), _t(q, dev), dict(cap=CAP, q=q), "scan_heads_softcap"


@functools.lru_cache(maxsize=2)
def _scaled_q(case, H, Hkv):
    return lc.scaled_q(case, sc.CAPS[0] / 2, H, Hkv)


def _counts():
    from min_llm_inference_amd import ops
    return {f: ops.launch_count(f) for f in SCAN_FAMILIES}


def _lean_twice(mli, dev, x, elem, what, want_counts, entry="scan", extra=(), H=1, q=None):
    """Two launches with equal bits, the counters zero after each, the launch counters as wanted (per launch); returns the
    result on the host."""
    from min_llm_inference_amd import ops
    c = x.case
    ops.reset_launch_counts()
    res = []
    for _ in range(2):
        out = torch.full((c.B, c.D), lc.SENTINEL, device=dev)
        assert _call(mli, dev, x, entry, extra, elem, out, H=H, q=q) == 0, what
        res.append(host(out).copy())
        _counters_are_zero(_WS["ws"], what)
    assert_equal(res[1], res[0], what=f"{what}: second launch")
    got = _counts()
    want = {f: 2 * want_counts.get(f, 0) for f in SCAN_FAMILIES}
    assert got == want, f"{what}: launch counters {got}, wanted {want}"
    faults = lc.whole_output_faults(c, res[0])
    assert not faults, f"{what}: " + "; ".join(faults)
    return res[0]


def _judge(oracle, x, got, rows, path, elem, H=1, Hkv=None, window=0, sinks=0, **biased):
    """asserts; returns {family: tolerance}"""
    res = lc.judge_rows(oracle, x.case, x.values_of, got, rows, H, Hkv, window, sinks, **biased)
    failures = []
    tols = {}
    for family, (err, e_or) in sorted(res.items()):
        ck = Checker(family, elem)
        ck.check(path, "attention", np.asarray(err), np.asarray(e_or))
        failures += ck.failures
        tols[family] = fm.tolerance(np.asarray(e_or))
        if biased.get("sink") is not None:
            SINK_RATIOS.append(float(np.max(err)) / tols[family])
    assert not failures, "\n".join(failures)
    return tols


# ---- single-head chunked scan: rows ------------------------------------------------------------------------------------------
def _rows_lengths(B):
    """rows 0, 8191 and 16383 (and B - 1) with 127 tokens, a band of lengths around the item size, the rest 0 .. 40"""
    rng = np.random.default_rng(4100)
    L = rng.integers(0, 41, size=B).astype(np.int32)
    L[rng.random(B) < 0.3] = 0
    named = {0: 127, 8191: 127, 16383: 127, B - 1: 127, 1: 0, 2: 63, 3: 64, 4: 65, 5: 1, 6: 126, 16382: 64, 16381: 0, 8192: 80}
    band = rng.choice(np.arange(16, 16000), size=200, replace=False)      # rows with a second item all over the batch
    L[band] = rng.integers(64, 128, size=200)
    for b, n in named.items():
        L[b] = n
    return L, sorted(named) + sorted(int(b) for b in band[:16])


@functools.lru_cache(maxsize=1)
def _rows_case(B):
    L, named = _rows_lengths(B)
    fams = {0: "early_peak", 16383: "late_peak", 8191: "offset-", 6: "late_peak", 8192: "early_peak"}
    return lc.SparseCase(4101, L, 128, 64, families=fams), named


ROWS_ELEMS = ("f32", "bf16", "fp8")


def _materialising(mli, dev, oracle, x, elem, rows, what, path):
    """phases 3: probabilities with an exactly zero tail in qkt_output, attention_result; judged on `rows`"""
    c = x.case
    out = torch.full((c.B, c.D), lc.SENTINEL, device=dev)
    qkt = torch.full((c.B, c.S), lc.SENTINEL, device=dev)
    assert _call(mli, dev, x, "scan", (), elem, out, qkt=qkt, phases=3) == 0, what
    got = host(out).copy()
    # the second launch: the same bits in attention_result and in every probability
    out2 = torch.full((c.B, c.D), lc.SENTINEL, device=dev)
    qkt2 = torch.full((c.B, c.S), lc.SENTINEL, device=dev)
    assert _call(mli, dev, x, "scan", (), elem, out2, qkt=qkt2, phases=3) == 0, what
    assert torch.equal(out.view(torch.int32), out2.view(torch.int32)), f"{what}: second launch, attention_result"
    assert torch.equal(qkt.view(torch.int32), qkt2.view(torch.int32)), f"{what}: second launch, qkt_output"
    del out2, qkt2
    faults = lc.whole_output_faults(c, got)
    assert not faults, f"{what}: " + "; ".join(faults)
    _judge(oracle, x, got, rows, path, elem)
    idx = _t(np.asarray(rows), dev)
    p = host(qkt[idx])
    res = {}
    for i, b in enumerate(rows):
        err, e_or = res.setdefault(c.family(b), ([], []))
        n = int(c.lengths[b])
        if n == 0:
            err.append(np.inf if p[i].any() else 0.0)
            e_or.append(0.0)
            continue
        K, V = x.values_of(b)
        _, model, (_, po, _) = lc.row_truth(oracle, c.q[b], K, V)[0]
        err.append(np.inf if p[i, n:].any() else float(fm.probability_error(p[i:i + 1, :n], model)[0]))
        e_or.append(float(fm.probability_error(po, model)[0]))
    failures = []
    for family, (err, e_or) in sorted(res.items()):
        ck = Checker(family, elem)
        ck.check(path, "probabilities", np.asarray(err), np.asarray(e_or))
        failures += ck.failures
    assert not failures, "\n".join(failures)
    # every row's tail, judged or not: exact zeros beyond the length
    tail = (torch.arange(c.S, device=dev)[None, :] >= x.L[:, None]) & (qkt != 0)
    assert not bool(tail.any()), f"{what}: the probabilities' tail is not zero"
    return got


@pytest.mark.parametrize("elem", ROWS_ELEMS)
def test_chunked_scan_on_the_last_arrival_counter(oracle, mli, dev, elem):
    """(16384, 128, 64), chunk_tokens 64: two items per row, row 16383 merges on the last arrival counter.  Judged: the named
    rows (0, 8191, 16383, lengths 0, 1, 63 .. 65, 126, 127) and a fixed random sample of 64; every row is checked for
    sentinel, NaN and the zero of an empty row.  fp32 / bf16 also in the materialising form (phases 3)."""
    case, named = _rows_case(16384)
    x = _pages(case, elem, dev)
    rows = lc.sample_rows(case.B, named)
    try:
        _tune(mli, chunk_tokens=64)
        got = _lean_twice(mli, dev, x, elem, f"B 16384 {elem}", {"scan_chunked": 1})
        _judge(oracle, x, got, rows, "limits: chunked scan, B 16384", elem)
        if elem != "fp8":
            _materialising(mli, dev, oracle, x, elem, rows, f"B 16384 {elem} phases 3", "limits: chunked scan, B 16384, phases 3")
            _counters_are_zero(_WS["ws"], "phases 3")
    finally:
        _tune(mli, **DEFAULTS)


@pytest.mark.parametrize("elem", ROWS_ELEMS)
def test_chunked_scan_beyond_the_arrival_counters(oracle, mli, dev, elem):
    """(16385, 128, 64): more rows than counters -- the lean scan hands the merge to the combine launch and is still right;
    the counter region stays zero.  Judged: the named rows, row 16384 and a sample of 64."""
    case, named = _rows_case(16385)
    x = _pages(case, elem, dev)
    try:
        _tune(mli, chunk_tokens=64)
        got = _lean_twice(mli, dev, x, elem, f"B 16385 {elem}", {"scan_chunked": 1})
        _judge(oracle, x, got, lc.sample_rows(case.B, named), "limits: chunked scan, B 16385", elem)
    finally:
        _tune(mli, **DEFAULTS)


# ---- single-head chunked scan: width -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _wide_case(D, flat=False):
    return lc.wide_case(D, flat)


WIDE_SHAPES = [("f32", 2048), ("bf16", 4096), ("fp8", 2048)]


@pytest.mark.parametrize("elem,D", WIDE_SHAPES)
def test_widest_rows(oracle, mli, dev, elem, D):
    """the widest rows each page type takes: eight lane loads split over the waves (fp32, bf16), two for fp8.  All rows judged."""
    x = _pages(_wide_case(D), elem, dev)
    rows = list(range(8))
    got = _lean_twice(mli, dev, x, elem, f"D {D} {elem}", {"scan_chunked": 1})
    _judge(oracle, x, got, rows, "limits: widest rows", elem)
    if elem != "fp8":
        _materialising(mli, dev, oracle, x, elem, rows, f"D {D} {elem} phases 3", "limits: widest rows, phases 3")


# ---- single-head chunked scan: length ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _longest_case(family):
    return lc.SparseCase(4300, [0, 65535, 1], 65536, 64, families={1: family})


LONG_FAMILIES = ("flat", "early_peak", "late_peak", "offset-")


@pytest.mark.parametrize("ct", [64, 1024])
@pytest.mark.parametrize("family", LONG_FAMILIES)
def test_longest_rows_lean(oracle, mli, dev, family, ct):
    """(3, 65536, 64), lengths 0, 65535, 1, items of 64 (1025 grid rows, 1024 pairs merged) and 1024 (65 grid rows), on
    every page type.  All rows judged."""
    case = _longest_case(family)
    try:
        _tune(mli, chunk_tokens=ct)
        for elem in ("f32", "bf16", "fp8"):
            x = _pages(case, elem, dev)
            got = _lean_twice(mli, dev, x, elem, f"S 65536 ct {ct} {elem} {family}", {"scan_chunked": 1})
            _judge(oracle, x, got, [0, 1, 2], f"limits: longest rows, items of {ct}", elem)
    finally:
        _tune(mli, **DEFAULTS)


@pytest.mark.parametrize("ct", [64, 1024])
def test_longest_rows_materialising(oracle, mli, dev, ct):
    """the same rows through phases 1 (raw scores) and phases 3 (probabilities with an exactly zero tail, attention), fp32
    and bf16.  All rows judged."""
    case = _longest_case("late_peak")
    try:
        _tune(mli, chunk_tokens=ct)
        for elem in ("f32", "bf16"):
            x = _pages(case, elem, dev)
            out = torch.full((3, 64), lc.SENTINEL, device=dev)
            qkt = torch.full((3, 65536), lc.SENTINEL, device=dev)
            assert _call(mli, dev, x, "scan", (), elem, out, qkt=qkt, phases=1) == 0
            raw = host(qkt).copy()
            qkt.fill_(lc.SENTINEL)
            assert _call(mli, dev, x, "scan", (), elem, out, qkt=qkt, phases=1) == 0
            assert host(qkt).tobytes() == raw.tobytes(), "phases 1: second launch"
            K, V = x.values_of(1)
            _, model, (xo, _, _) = lc.row_truth(oracle, case.q[1], K, V)[0]
            ck = Checker("late_peak", elem)
            ck.check(f"limits: longest rows, items of {ct}", "scores", fm.score_error(raw[1:2, :65535], model), fm.score_error(xo, model))
            ck.done()
            _materialising(mli, dev, oracle, x, elem, [0, 1, 2], f"S 65536 ct {ct} {elem} phases 3",
                           f"limits: longest rows, items of {ct}, phases 3")
    finally:
        _tune(mli, **DEFAULTS)


# ---- single-head chunked scan: row order -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _order_case(B, S, order):
    top = S - 1 if S <= 1024 else 1023
    if order == "descending":
        L = np.linspace(top, 0, B).astype(np.int32)
    elif order == "ascending":
        L = np.linspace(0, top, B).astype(np.int32)
    else:
        L = np.full(B, top - 16, np.int32)
    return lc.SparseCase(4400 + B, L, S, 64)


# (B, S, chunk_tokens, the rows counter that must move: ordered / grid / neither)
ORDER_SHAPES = [(512, 64, 0, "scan_rows_grid_order"), (513, 64, 0, "scan_rows_ordered"), (2048, 64, 0, "scan_rows_ordered"),
                (2049, 64, 0, "scan_rows_grid_order"), (600, 1024, 1024, "scan_rows_ordered"), (600, 1040, 1024, None)]


@pytest.mark.parametrize("order", ["descending", "ascending", "equal"])
@pytest.mark.parametrize("B,S,ct,family", ORDER_SHAPES)
def test_row_order_frontier(oracle, mli, dev, B, S, ct, family, order):
    """The longest-first hand-out on both sides of its three bounds (more than 512 rows, at most 2048, at most 64 live pages),
    lengths descending, ascending and all equal; scan_rows_ordered against scan_rows_grid_order says which ran.  S 64: every
    row judged; S 1024 / 1040: rows 0, B / 2, B - 1 and a fixed sample of 64."""
    case = _order_case(B, S, order)
    rows = list(range(B)) if S == 64 else lc.sample_rows(B, [0, B // 2, B - 1])
    want = {"scan_chunked": 1}
    if family:
        want[family] = 1
    try:
        _tune(mli, chunk_tokens=ct)
        for elem in ("f32", "bf16", "fp8"):
            x = _pages(case, elem, dev)
            got = _lean_twice(mli, dev, x, elem, f"({B}, {S}) {order} {elem}", want)
            _judge(oracle, x, got, rows, f"limits: row order ({B}, {S})", elem)
    finally:
        _tune(mli, **DEFAULTS)


# ---- equal-shares scan -------------------------------------------------------------------------------------------------------
def _sparse_lengths(seed, B, S):
    """a handful of rows of S - 1, S / 2 and page-boundary lengths, the rest 0 .. 40 tokens (a third of them empty)"""
    rng = np.random.default_rng(seed)
    L = rng.integers(0, 41, size=B).astype(np.int32)
    L[rng.random(B) < 0.33] = 0
    named = {0: S - 1, B // 2: S // 2, B - 1: S - 17, 1: 0, 2: 16, 3: 17, 4: 15, B - 2: 48, B - 3: 33, 5: 1}
    for b, n in named.items():
        L[b] = n
    return L, sorted(named)


@functools.lru_cache(maxsize=2)
def _shares_case(B, S, D):
    L, named = _sparse_lengths(4500 + B + S, B, S)
    fams = {0: "early_peak", B - 1: "late_peak", B // 2: "offset-"}
    return lc.SparseCase(4501 + D, L, S, D, families=fams), named


def _the_triples_are_those_of_the_restated_pieces(oracle, x, dev, rows, what):
    """tests/test_stream_partition_gpu.py's per-slot comparison on sparse rows: the maxima the launch left in its workspace
    against the maxima of the restated pieces, for the rows of `rows` that lie in two or more pieces"""
    c = x.case
    G_launch = 2 * torch.cuda.get_device_properties(dev).multi_processor_count
    pt = sm.partition(c.lengths, c.S, G_launch, 4, 64)
    per_row = -(-c.S // 64)
    ws = _WS["ws"]
    n = 0
    for b in rows:
        if pt.row_pieces[b] < 2:
            continue
        K, V = x.values_of(b)
        _, model, (xo, _, _) = lc.row_truth(oracle, c.q[b], K, V)[0]
        tol_x = fm.tolerance(fm.score_error(xo, model))
        want = []
        for lo, hi, _ in pt.pieces:
            if min(pt.start[b + 1], hi) > max(pt.start[b], lo):
                t0 = (max(int(pt.start[b]), lo) - int(pt.start[b])) * 16
                t1 = min((min(int(pt.start[b + 1]), hi) - int(pt.start[b])) * 16, int(c.lengths[b]))
                want.append(float(model.x[0, t0:t1].max()))
        assert len(want) == pt.row_pieces[b] <= per_row
        off = lc.COUNTER_BYTES + b * per_row * 8
        ml = host(ws[off:off + len(want) * 8]).view(np.float32).reshape(-1, 2)
        worst = float(np.abs(ml[:, 0].astype(np.float64) - np.asarray(want)).max()) / model.x_scale[0]
        assert worst <= tol_x, f"{what}: row {b}: the workspace does not hold the maxima of the restated pieces ({worst:.3e} > {tol_x:.3e})"
        n += 1
    assert n > 0, f"{what}: no judged row lies in two pieces"
    print(f"TRIPLES {what}: {n} rows hold the maxima of the restated pieces")


# (B, S, D, scan_stream_min_tokens, equal shares?)
SHARES = [(2048, 1024, 64, 1 << 21, True), (2049, 1024, 64, 1 << 21, False), (2047, 1024, 64, 1 << 21, False),
          (2048, 1024, 64, 0, True), (2048, 1008, 64, 0, False), (256, 8192, 64, 1 << 21, True), (256, 8256, 64, 1 << 21, False)]


def _shares(oracle, mli, dev, B, S, D, min_tokens, near, elems, path):
    case, named = _shares_case(B, S, D)
    rows = lc.sample_rows(B, named)
    try:
        _tune(mli, scan_stream_min_tokens=min_tokens)
        for elem in elems:
            x = _pages(case, elem, dev)
            what = f"({B}, {S}, {D}) {elem} min_tokens {min_tokens}"
            got = _lean_twice(mli, dev, x, elem, what, {"scan_equal_shares": 1} if near else {"scan_chunked": 1})
            _judge(oracle, x, got, rows, path + (", equal shares" if near else ", chunked"), elem)
            if near:
                _the_triples_are_those_of_the_restated_pieces(oracle, x, dev, rows, what)
    finally:
        _tune(mli, **DEFAULTS)


@pytest.mark.parametrize("B,S,D,min_tokens,near", SHARES)
def test_equal_shares_frontier(oracle, mli, dev, B, S, D, min_tokens, near):
    """The equal-shares scan at its last rows (2048), its first n_batch x n_sequence (2^21 under the default knob), its
    shortest n_sequence (1024) and the longest whose statistics fit the q buffer (fp32, emb_dim 64: 8192), and the chunked
    scan one step beyond each; launch counters say which ran, and on the near side the workspace holds the maxima of the
    restated pieces.  Judged: the named rows (S - 1, S / 2, page-boundary lengths, 0, 1) and a fixed sample of 64."""
    _shares(oracle, mli, dev, B, S, D, min_tokens, near, ("f32",) if S > 1024 else ("f32", "bf16", "fp8"), "limits: equal shares frontier")


LDS_SIDES = ["inside", "beyond"]


@pytest.mark.parametrize("side", LDS_SIDES)
@pytest.mark.parametrize("D,elem", [(512, "f32"), (512, "bf16"), (512, "fp8"), (1024, "bf16")])
def test_equal_shares_lds_frontier(oracle, mli, dev, D, elem, side):
    """n_batch 2048 at the longest n_sequence whose dynamic LDS stays within 80 KiB -- between 64 and 80 KiB the launcher
    raises the kernel's limit first -- and at the first beyond it, where the chunked scan runs.  The lengths come from the
    restated sum (limit_cases.stream_lds_bytes) at this device's CU count; the launch counter judges the restatement too.
    emb_dim 1024 bf16 is the two-lane-load kernel (MAXSEG 2).  Judged: the named rows and a fixed sample of 64."""
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    S_in, S_out = lc.stream_lds_frontier(2048, D, elem, n_cu)
    print(f"LDS frontier at {n_cu} CUs: S {S_in} -> {lc.stream_lds_bytes(2048, S_in, D, elem, n_cu)} B, "
          f"S {S_out} -> {lc.stream_lds_bytes(2048, S_out, D, elem, n_cu)} B")
    _shares(oracle, mli, dev, 2048, S_in if side == "inside" else S_out, D, 1 << 21, side == "inside", (elem,), "limits: equal shares LDS")


# ---- multi-head family -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _heads_case(D):
    return lc.heads_case(D)


# (entry point, arguments behind emb_dim, emb_dim, H, Hkv, W, K)
HEAD_FORMS = {"heads": ("heads", (2,), 128, 2, 2, 0, 0), "window": ("window", (2, 17), 128, 2, 2, 17, 0),
              "sinks": ("sinks", (2, 16, 4), 128, 2, 2, 16, 4), "gqa": ("gqa", (2, 1, 0, 0), 128, 2, 1, 0, 0),
              "window_one_head": ("window", (1, 17), 64, 1, 1, 17, 0), "sinks_one_head": ("sinks", (1, 16, 4), 64, 1, 1, 16, 4),
              # the biased and the capped scan: separate instantiations of heads_scan_item (arguments: _biased)
              "alibi": ("alibi", None, 128, 2, 2, 0, 0), "alibi_gqa": ("alibi", None, 128, 2, 1, 0, 0),
              "alibi_sinks": ("alibi", None, 128, 2, 2, 16, 4),
              "softcap": ("softcap", None, 128, 2, 2, 0, 0), "softcap_gqa": ("softcap", None, 128, 2, 1, 0, 0),
              "softcap_window": ("softcap", None, 128, 2, 2, 17, 0),
              # the scan with sink logits: its plain, grouped, windowed and sinks kernels (three differently templated ones)
              "sink_logits": ("sink_logits", None, 128, 2, 2, 0, 0), "sink_logits_gqa": ("sink_logits", None, 128, 2, 1, 0, 0),
              "sink_logits_window": ("sink_logits", None, 128, 2, 2, 17, 0), "sink_logits_sinks": ("sink_logits", None, 128, 2, 2, 16, 4)}


@pytest.mark.parametrize("elem", ["f32", "bf16"])
@pytest.mark.parametrize("form", sorted(HEAD_FORMS))        # HEAD_FORMS
def test_heads_family_on_the_last_row(oracle, mli, dev, form, elem):
    """(16384, 64, 128) with two heads -- plain, W 17, (W 16, K 4), one K/V head -- and (16384, 64, 64) with one head under
    a window, with and without sinks: the last batch the plans accept.  Judged: the named rows (0, 8191, 16383 with 63
    tokens; lengths 0, 1, 16 .. 18, 20, 21, 33 around the window and sink edges) and a fixed sample of 64."""
    entry, extra, D, H, Hkv, W, K = HEAD_FORMS[form]
    case, named = _heads_case(D)
    x = _pages(case, elem, dev)
    counter, q, kw = "scan_heads_window", None, {}
    rows = lc.sample_rows(case.B, named)
    if extra is None:
        extra, q, kw, counter = _biased(entry, case, H, Hkv, W, K, dev, x=x, rows=rows)
    got = _lean_twice(mli, dev, x, elem, f"{form} {elem}", {counter: 1}, entry=entry, extra=extra, H=H, q=q)
    _judge(oracle, x, got, rows, f"limits: B 16384, {form}", elem, H=H, Hkv=Hkv, window=W, sinks=K, **kw)


@pytest.mark.parametrize("elem", ["f32", "bf16"])
def test_heads_on_the_last_arrival_counter(oracle, mli, dev, elem):
    """The rows of test_chunked_scan_on_the_last_arrival_counter, (16384, 128, 64), read as two heads of 32 columns at
    chunk_tokens 64 -- two items per row, so that row 16383 merges per head on the last arrival counter -- plain and under
    W 100 (a span of 128 tokens: two items too).  Judged: the named rows and a fixed sample of 64."""
    case, named = _rows_case(16384)
    x = _pages(case, elem, dev)
    rows = lc.sample_rows(case.B, named)
    try:
        _tune(mli, chunk_tokens=64)
        for entry, extra, W in (("heads", (2,), 0), ("window", (2, 100), 100), ("window", (1, 100), 100), ("alibi", None, 0),
                                ("softcap", None, 0), ("alibi", None, 100), ("softcap", None, 100)):
            counter, q, kw = "scan_heads_window", None, {}
            if extra is None:
                extra, q, kw, counter = _biased(entry, case, 2, 2, W, 0, dev)
            H = extra[0]
            got = _lean_twice(mli, dev, x, elem, f"B 16384 {entry} H {H} W {W} {elem}", {counter: 1}, entry=entry, extra=extra, H=H, q=q)
            _judge(oracle, x, got, rows, f"limits: B 16384, two items, {entry} H {H} W {W}", elem, H=H, window=W, **kw)
    finally:
        _tune(mli, **DEFAULTS)


@functools.lru_cache(maxsize=1)
def _merge_case():
    return lc.merge_case()


MERGE_FORMS = ["heads", "window", "alibi", "softcap", "sink_logits", "sink_logits_window"]


@pytest.mark.parametrize("form", MERGE_FORMS)
def test_merge_statistics_fill_their_lds(oracle, mli, dev, form):
    """bf16 (2, 16384, 1024) with 32 heads: the plan raises the item size to 128 and the last arriver stages 128 x 32 = 4096
    pairs, all the LDS the merge has; plain and under W 8192.  early_peak on odd heads, late_peak on even ones.  Both rows
    judged, head by head.
    With sink logits the last arriver loops over 128 published pairs per head and adds the sink exactly once; the 32 logits
    come from the two judged rows, head by head.  A second launch takes the logits of heads 8 .. 31 rotated by one (head h is
    given the logit of head h + 1, head 31 that of head 8) and those of heads 0 .. 7 untouched: heads 0 .. 7 keep their bits and
    every one of heads 8 .. 31 moves by more than the tolerance on both rows -- a kernel that read the logit of a neighbouring
    head, or of head h mod 8, could not pass both launches."""
    x = _pages(_merge_case(), "bf16", dev)
    entry, extra, W = {"heads": ("heads", (32,), 0), "window": ("window", (32, 8192), 8192),
                       "sink_logits_window": ("sink_logits", None, 8192)}.get(form, (form, None, 0))
    counter, q, kw = "scan_heads_window", None, {}
    if extra is None:
        extra, q, kw, counter = _biased(entry, x.case, 32, 32, W, 0, dev, x=x, rows=[0, 1])
    got = _lean_twice(mli, dev, x, "bf16", f"32 heads {form}", {counter: 1}, entry=entry, extra=extra, H=32, q=q)
    tols = _judge(oracle, x, got, [0, 1], f"limits: 32 heads, {form}", "bf16", H=32, window=W, **kw)
    if entry != "sink_logits":
        return
    z = kw["sink"]
    turned = z.copy()
    turned[8:] = np.roll(z[8:], -1)
    assert (turned[:8] == z[:8]).all() and (turned[8:] != z[8:]).all() and turned[31] == z[8] and turned[8] == z[9]
    other = _lean_twice(mli, dev, x, "bf16", f"32 heads {form}, logits of heads 8 .. 31 rotated", {counter: 1}, entry=entry,
                        extra=extra[:4] + (_t(turned, dev),), H=32)
    hd = x.case.D // 32
    assert_equal(other[:, :8 * hd], got[:, :8 * hd], what="heads 0 .. 7 under the rotated logits")
    for b in (0, 1):
        K, V = x.values_of(b)
        for h, (cols, model, _) in enumerate(lc.row_truth(oracle, x.case.q[b], K, V, 32, 32, W, 0, sink=z)):
            if h >= 8:
                moved = float(np.abs(other[b, cols].astype(np.float64) - got[b, cols]).max() / model.o_scale[0])
                assert moved > tols[x.case.family(b, h)], f"row {b} head {h}: the rotated logits move the result by {moved:.3e} only"


@functools.lru_cache(maxsize=1)
def _family_case(pair):
    return lc.sink_family_case(pair)


SINK_PAIRS = list(lc.SINK_FAMILY_PAIRS)


@pytest.mark.parametrize("elem", ["bf16", "f32"])
@pytest.mark.parametrize("pair", SINK_PAIRS, ids=["-".join(p) for p in SINK_PAIRS])
def test_score_families_against_the_sink(oracle, mli, dev, pair, elem):
    """(24, 1024, 256) with 8 heads on 2 K/V heads at chunk_tokens 64 -- 16 items per row, the sink added once by the last
    arriver -- on rows of 1, 63, 64, 65, 1008, 1023, 0 and random lengths whose K/V heads carry the score families two by two
    (flat and peaked, offset+ and offset-, late_peak and early_peak; a group's query heads score 1, 1.125, 1.25 and 1.375 times
    the first): rows whose own scores sit at +-200 or carry a peak 30 high in their first or last page, where the items' maxima
    and the sink's logit lie far apart.  Two launches, all rows judged:
      1. the logits learned per head from what the pages hold (the condition on them asserted): the model;
      2. z = 0 on every head, the "off-by-one" softmax: the offset+ heads give the bits of mli_decode_scan_paged_gqa (expf of
         -200 and less is 0), the offset- heads are finite and at most exp(-150) max|V| in magnitude, the others the model."""
    case = _family_case(pair)
    x = _pages(case, elem, dev)
    rows = list(range(case.B))
    H, Hkv, hd = 8, 2, 32
    what = f"families {'/'.join(pair)} {elem}"
    try:
        _tune(mli, chunk_tokens=64)
        plain = _lean_twice(mli, dev, x, elem, what + " gqa", {"scan_heads_window": 1}, entry="gqa", extra=(H, Hkv, 0, 0), H=H)
        extra, _, kw, counter = _biased("sink_logits", case, H, Hkv, 0, 0, dev, x=x, rows=rows)
        got = _lean_twice(mli, dev, x, elem, what + " learned", {counter: 1}, entry="sink_logits", extra=extra, H=H)
        _judge(oracle, x, got, rows, f"limits: score families against the sink, {'/'.join(pair)}", elem, H=H, Hkv=Hkv, **kw)
        live = case.lengths > 0
        assert np.abs(got - plain)[live].max() > 1e-3, f"{what}: the logits change nothing"
        zero = np.zeros(H, np.float32)
        got0 = _lean_twice(mli, dev, x, elem, what + " z = 0", {counter: 1}, entry="sink_logits", extra=(H, Hkv, 0, 0, _t(zero, dev)), H=H)
        fams = [case.family(rows[0], h) for h in range(H)]
        top_v = max(float(np.abs(x.values_of(b)[1]).max()) for b in rows if case.lengths[b])
        for h, family in enumerate(fams):
            cols = slice(h * hd, (h + 1) * hd)
            if family == "offset+":
                assert_equal(got0[:, cols], plain[:, cols], what=f"{what}: z = 0 on offset+ head {h} against the _gqa call")
            elif family == "offset-":
                assert np.isfinite(got0[:, cols]).all() and np.abs(got0[:, cols]).max() <= np.exp(-150.0) * top_v, \
                    f"{what}: z = 0 on offset- head {h}: {np.abs(got0[:, cols]).max():.3e}"
        rest = [h for h, family in enumerate(fams) if not family.startswith("offset")]
        if rest:
            _judge(oracle, x, got0, rows, f"limits: score families against the sink, {'/'.join(pair)}, z = 0", elem, H=H, Hkv=Hkv,
                   sink=zero, heads=rest)
    finally:
        _tune(mli, **DEFAULTS)


# ---- contiguous scan ---------------------------------------------------------------------------------------------------------
CONTIGUOUS_SHAPES = [(8192, 512, 16), (2, 131072, 16), (2, 512, 13052), (12, 256, 16), (12, 260, 16)]


@pytest.mark.parametrize("B,S,D", CONTIGUOUS_SHAPES)
def test_contiguous_scan_frontier(oracle, mli, dev, B, S, D):
    """mli_decode_scan_contiguous at its last batch with several chunks per row (8192: half the arrival counters), at its
    longest row (512 chunks of 256 tokens: every pair the 4 KiB buffer of the merge holds), at its widest row (emb_dim 13052:
    64 KiB of LDS less 4 bytes), and on both sides of kNvChunk (n_sequence 256: one item per row; 260: two and the merge).  Caches are generated on the
    device; the judged rows -- first, last and a fixed sample of 64 -- are copied out, get the finite dead-slot poison, and
    go back."""
    gen = torch.Generator(device=dev).manual_seed(4800 + B)
    kt = torch.rand((B, D, S), generator=gen, device=dev) * 2 - 1
    v = torch.rand((B, S, D), generator=gen, device=dev) * 2 - 1
    q = torch.rand((B, D), generator=gen, device=dev) * 2 - 1
    L = np.random.default_rng(4801).integers(0, S, size=B).astype(np.int32)
    L[0], L[B - 1] = S - 1, S - 1 if B > 2 else min(70000, S - 2)
    rows = lc.sample_rows(B, [0, B - 1] + ([1, 2, 3, 4] if B > 2 else []))
    if B > 2:
        L[1], L[2], L[3], L[4] = 0, min(256, S - 1), min(257, S - 1), 255
    idx = _t(np.asarray(rows), dev)
    qh, kth, vh, Lh = host(q[idx]).copy(), host(kt[idx]).copy(), host(v[idx]).copy(), L[rows]
    poison_contiguous(qh, kth, vh, Lh)
    kt[idx], v[idx] = _t(kth, dev), _t(vh, dev)
    Ld = _t(L, dev)
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ws[:lc.COUNTER_BYTES] = 0
    res = []
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    for _ in range(2):
        out = torch.full((B, D), lc.SENTINEL, device=dev)
        assert mli.mli_decode_scan_contiguous(p(q), p(kt), p(v), p(Ld), p(out), B, S, D, p(ws), need,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        res.append(host(out).copy())
        _counters_are_zero(ws, f"contiguous ({B}, {S}, {D})")
    assert_equal(res[1], res[0], what="second launch")
    got = res[0]
    assert np.isfinite(got).all() and not (got == lc.SENTINEL).any() and not got[L == 0].any()
    from accuracy_cases import oracle_scan
    model = fm.Model(qh, kth, vh, Lh)
    ck = Checker("flat", "f32")
    ck.check(f"limits: contiguous scan ({B}, {S}, {D})", "attention", fm.attention_error(got[rows], model),
             fm.attention_error(oracle_scan(oracle, qh, kth, vh, Lh)[2], model))
    ck.done()


# ---- offsets beyond 2^31 -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _offsets_case():
    B, S, D = 16384, 4096, 2048
    L = np.zeros(B, np.int32)
    L[16380:] = [S - 1, S // 2, 65, 64]
    return lc.SparseCase(4900, L, S, D, families={16380: "late_peak", 16381: "early_peak"})


def _needs(dev, n_bytes, what):
    free, total = torch.cuda.mem_get_info(dev)
    if free < 2 * n_bytes:
        pytest.skip(f"{what} needs {n_bytes / 2 ** 30:.1f} GiB of device memory; {free / 2 ** 30:.1f} of {total / 2 ** 30:.1f} GiB are free")


@pytest.mark.parametrize("phases", [7, 3])
def test_offsets_beyond_2_31_paged(oracle, mli, dev, phases):
    """fp32 (16384, 4096, 2048), chunk_tokens 64: the partial rows are 2^31 floats (8 GiB) and only rows 16380 .. 16383 are
    live (S - 1, S / 2, 65, 64 tokens), so every offset they use lies beyond 2^31 elements.  Lean and materialising.  Judged:
    the four live rows and rows 0 and 16379; every row is checked for sentinel, NaN and zeros.  Skips when less than twice
    the workspace is free."""
    case = _offsets_case()
    need = int(mli.mli_attention_workspace_bytes(case.B, case.S, case.D))
    assert need > 8 << 30
    if _WS.get("ws") is None or _WS["ws"].numel() < need:
        _WS.pop("ws", None)
        torch.cuda.empty_cache()
        _needs(dev, need + (case.B * case.S * 4 if phases == 3 else 0), "the workspace of (16384, 4096, 2048)")
    x = _pages(case, "f32", dev)
    rows = [0, 16379, 16380, 16381, 16382, 16383]
    try:
        _tune(mli, chunk_tokens=64)
        if phases == 7:
            got = _lean_twice(mli, dev, x, "f32", "offsets beyond 2^31, lean", {"scan_chunked": 1})
            _judge(oracle, x, got, rows, "limits: offsets beyond 2^31, lean", "f32")
        else:
            _materialising(mli, dev, oracle, x, "f32", rows, "offsets beyond 2^31, phases 3", "limits: offsets beyond 2^31, phases 3")
            _counters_are_zero(_WS["ws"], "phases 3")
    finally:
        _tune(mli, **DEFAULTS)


@pytest.mark.parametrize("ct", [64])
def test_offsets_beyond_2_31_three_stage(oracle, mli, dev, ct):
    """The standalone launchers at the same shape and item size: mli_qkt_paged, mli_softmax_in_place_with_lengths and
    mli_softmax_v_paged, whose partial sums are 2^31 floats.  Judged: probabilities (zero tail) and attention of the four
    live rows and of rows 0 and 16379."""
    case = _offsets_case()
    need = int(mli.mli_attention_workspace_bytes(case.B, case.S, case.D))
    if _WS.get("ws") is None or _WS["ws"].numel() < need:
        _WS.pop("ws", None)
        torch.cuda.empty_cache()
        _needs(dev, need + case.B * case.S * 4, "the workspace of (16384, 4096, 2048)")
    x = _pages(case, "f32", dev)
    rows = [0, 16379, 16380, 16381, 16382, 16383]
    ws, need = _workspace(mli, dev, case.B, case.S, case.D)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out = torch.full((case.B, case.D), lc.SENTINEL, device=dev)
    qkt = torch.zeros((case.B, case.S), device=dev)
    first = None
    try:
        _tune(mli, chunk_tokens=ct)
        for _ in range(2):      # twice: the same bits in the probabilities and in attention_result
            out.fill_(lc.SENTINEL)
            qkt.zero_()
            assert mli.mli_qkt_paged(p(x.q), p(x.table), p(x.L), p(qkt), case.B, case.S, case.D, st) == 0
            assert mli.mli_softmax_in_place_with_lengths(p(qkt), p(x.L), case.B, case.S, st) == 0
            assert mli.mli_softmax_v_paged(p(qkt), p(x.table), p(x.L), p(out), case.B, case.S, case.D, p(ws), need, st) == 0
            if first is None:
                first = (out.clone(), qkt.clone())
        assert torch.equal(first[0].view(torch.int32), out.view(torch.int32)), "second launch, attention_result"
        assert torch.equal(first[1].view(torch.int32), qkt.view(torch.int32)), "second launch, probabilities"
        first = None
    finally:
        _tune(mli, **DEFAULTS)
    got = host(out).copy()
    faults = lc.whole_output_faults(case, got)
    assert not faults, "; ".join(faults)
    _counters_are_zero(ws, "three-stage launchers")
    _judge(oracle, x, got, rows, "limits: offsets beyond 2^31, three-stage", "f32")
    probs = host(qkt[_t(np.asarray(rows), dev)])
    for i, b in enumerate(rows):
        n = int(case.lengths[b])
        assert not probs[i, n:].any(), f"row {b}: the tail is not zero"
        if n:
            K, V = x.values_of(b)
            _, model, (_, po, _) = lc.row_truth(oracle, case.q[b], K, V)[0]
            ck = Checker(case.family(b), "f32")
            ck.check("limits: offsets beyond 2^31, three-stage", "probabilities", fm.probability_error(probs[i:i + 1, :n], model),
                     fm.probability_error(po, model))
            ck.done()


def test_offsets_beyond_2_31_sampled_head(mli, dev):
    """mli_sample_tokens and mli_sample_tokens_logprobs on [16384, 131072] logits (2^31 floats): rows 16376 .. 16383 hold
    sampling_cases.drawn_case, then logprobs_model.families, and are judged against sampling_ref / logprobs_model; all other
    rows have length 0 (their logits are never read, their token is -1)."""
    import logprobs_model as lm
    import sampling_ref as ref
    from min_llm_inference_amd import ops
    from sampling_cases import drawn_case
    B, V, n = 16384, 131072, 8
    _WS.clear()
    torch.cuda.empty_cache()
    _needs(dev, B * V * 4 + int(mli.mli_sample_scratch_bytes(B, V)), "logits of [16384, 131072]")
    logits = torch.empty((B, V), device=dev)
    lengths = np.zeros(B, np.int32)
    par = lambda a, dt, fill: _t(np.concatenate([np.full(B - n, fill, dt), np.asarray(a, dt)]), dev)
    # tokens
    x, T, K, P, seed, L = drawn_case(np.random.default_rng(4950), n, V)
    logits[B - n:] = _t(x, dev)
    lengths[B - n:] = L
    args = (par(T, np.float32, 1.0), par(K, np.int32, 0), par(P, np.float32, 1.0), par(seed, np.int64, 1))
    got = host(ops.sample_tokens(logits, *args, _t(lengths, dev)))
    assert (got[:B - n] == -1).all()
    want, gap, margin = ref.sample(x, T, K, P, seed, L)
    posed = (gap > 1e-4) & (margin > 1e-4)
    print(f"SAMPLED rows {B - n} ..: got {got[B - n:].tolist()} want {want.tolist()} well posed {posed.tolist()}")
    assert posed.sum() >= 6 and (got[B - n:][posed] == want[posed]).all()
    for b in np.nonzero(~posed)[0]:
        assert ref.kept_set(x[b], T[b], K[b], P[b])[0][got[B - n + b]]
    # log-probabilities
    x, L = lm.families(V)
    logits[B - n:] = _t(np.array(x), dev)
    lengths[B - n:] = L
    tol = lm.tolerance(x)
    for T_, K_, P_ in ((0.0, 0, 1.0), (0.8, 40, 1.0)):
        args = (par(np.full(n, T_), np.float32, 1.0), par(np.full(n, K_), np.int32, 0), par(np.full(n, P_), np.float32, 1.0),
                par(np.arange(n) * 7919 + 11, np.int64, 1))
        plain = host(ops.sample_tokens(logits, *args, _t(lengths, dev)))
        tok, lp, ids, tops = [host(a) for a in ops.sample_tokens_logprobs(logits, *args, _t(lengths, dev), n_top=8)]
        assert tok.tobytes() == plain.tobytes() and (tok[:B - n] == -1).all() and (lp[:B - n] == -np.inf).all()
        err, tol2, bad = lm.compare((lp[B - n:], ids[B - n:], tops[B - n:]), x, tok[B - n:], 8)
        print(f"LOGPROBS rows {B - n} .. T {T_}: worst error {err:.3e} tol {tol:.3e}")
        assert tol2 == tol and not bad and err <= tol, (err, tol, bad)
    del logits
    torch.cuda.empty_cache()


def test_offsets_beyond_2_31_contiguous(oracle, mli, dev):
    """mli_decode_scan_contiguous on caches of 2049 x 256 x 4096 = 2^31 + 2^20 elements each: rows 2045 .. 2048 are live (4095,
    2048, 257, 256 tokens) with the finite dead-slot poison, all others have length 0 and are never read."""
    from accuracy_cases import oracle_scan
    B, S, D = 2049, 4096, 256
    _WS.clear()
    torch.cuda.empty_cache()
    _needs(dev, 2 * B * S * D * 4 + int(mli.mli_attention_workspace_bytes(B, S, D)), "two caches of (2049, 4096, 256)")
    kt = torch.empty((B, D, S), device=dev)
    v = torch.empty((B, S, D), device=dev)
    rows = [2045, 2046, 2047, 2048]
    L = np.zeros(B, np.int32)
    L[rows] = [S - 1, S // 2, 257, 256]
    rng = np.random.default_rng(4960)
    qh = (rng.random((4, D), dtype=np.float32) * 2 - 1).astype(np.float32)
    kth = (rng.random((4, D, S), dtype=np.float32) * 2 - 1).astype(np.float32)
    vh = (rng.random((4, S, D), dtype=np.float32) * 2 - 1).astype(np.float32)
    poison_contiguous(qh, kth, vh, L[rows])
    kt[rows[0]:] = _t(kth, dev)
    v[rows[0]:] = _t(vh, dev)
    q = torch.zeros((B, D), device=dev)
    q[rows[0]:] = _t(qh, dev)
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ws[:lc.COUNTER_BYTES] = 0
    Ld = _t(L, dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    res = []
    for _ in range(2):
        out = torch.full((B, D), lc.SENTINEL, device=dev)
        assert mli.mli_decode_scan_contiguous(p(q), p(kt), p(v), p(Ld), p(out), B, S, D, p(ws), need,
                                              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        res.append(host(out).copy())
        _counters_are_zero(ws, "contiguous caches beyond 2^31")
    assert_equal(res[1], res[0], what="second launch")
    got = res[0]
    assert np.isfinite(got).all() and not (got == lc.SENTINEL).any() and not got[:rows[0]].any()
    model = fm.Model(qh, kth, vh, L[rows])
    ck = Checker("flat", "f32")
    ck.check("limits: contiguous caches beyond 2^31", "attention", fm.attention_error(got[rows], model),
             fm.attention_error(oracle_scan(oracle, qh, kth, vh, L[rows])[2], model))
    ck.done()
    del kt, v
    torch.cuda.empty_cache()


# ---- window extremes ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _window_case(D=64, flat=False):
    return lc.window_case(D, flat)


# (entry point, W, K, windowed kernel?) on (12, 64, 64): the last windows the windowed kernels take, and the first hand-offs
WINDOW_CALLS = [("window", 1, 0, True), ("window", 63, 0, True), ("sinks", 59, 4, True), ("window", 64, 0, False), ("sinks", 60, 4, False)]


@pytest.mark.parametrize("entry,W,K,windowed", WINDOW_CALLS)
@pytest.mark.parametrize("elem,H", [("f32", 1), ("bf16", 1), ("fp8", 1), ("f32", 2), ("bf16", 2)])
def test_window_extremes(oracle, mli, dev, elem, H, entry, W, K, windowed):
    """(12, 64, 64): W 1 (V's newest row as the pages hold it), W S - 1 and K + W = S - 1 -- the last windows the windowed
    kernels take -- and W = S, K + W = S, which are the plain scan (one head: scan_chunked counts).  All rows judged."""
    case = _window_case()
    x = _pages(case, elem, dev)
    rows = list(range(case.B))
    extra = (H, W) if entry == "window" else (H, W, K)
    if windowed:
        want = {"scan_heads_window": 1}
    else:
        want = {"scan_chunked": 1, "scan_rows_grid_order": 1} if H == 1 else {"scan_heads_window": 1}
    got = _lean_twice(mli, dev, x, elem, f"{entry} W {W} K {K} H {H} {elem}", want, entry=entry, extra=extra, H=H)
    _judge(oracle, x, got, rows, f"limits: window extremes W {W} K {K} H {H}", elem, H=H, window=W if windowed else 0, sinks=K if windowed else 0)
    if W == 1:
        for b in rows:
            if case.lengths[b]:
                assert np.array_equal(got[b], x.values_of(b)[1][-1]), f"W 1: row {b} is not V's newest row"


BIASED_WINDOW_CALLS = [(e, W, K, w) for e in ("alibi", "softcap", "sink_logits")
                       for W, K, w in ((63, 0, True), (64, 0, False), (59, 4, True), (60, 4, False))] + [("sink_logits", 1, 0, True)]


@pytest.mark.parametrize("entry,W,K,windowed", BIASED_WINDOW_CALLS)
@pytest.mark.parametrize("elem", ["f32", "bf16"])
def test_window_extremes_biased(oracle, mli, dev, elem, entry, W, K, windowed):
    """test_window_extremes for the biased and the capped scan at two heads: W 63 and K 4 + W 59 are the last windows they take,
    W 64 and K 4 + W 60 the plain mask (the same kernel family counts either way: the result is the evidence).  All rows judged.
    With sink logits, on (12, 64, 128) without score families (one logit per head serves every row): both sides of the hand-off
    count as "scan_heads_sink_logits" -- the plain kind has its own sunk kernel --, the hand-offs give the bits of W 0 under the
    same logits, and W 1 is V's newest row times 1 / (1 + exp(z - x_newest)), computed here in float64 and held at the judge's
    tolerance."""
    sunk = entry == "sink_logits"
    case = _window_case(128, True) if sunk else _window_case()
    x = _pages(case, elem, dev)
    rows = list(range(case.B))
    extra, q, kw, counter = _biased(entry, case, 2, 2, W, K, dev, x=x, rows=rows)
    got = _lean_twice(mli, dev, x, elem, f"{entry} W {W} K {K} {elem}", {counter: 1}, entry=entry, extra=extra, H=2, q=q)
    tols = _judge(oracle, x, got, rows, f"limits: window extremes, {entry} W {W} K {K}", elem, H=2,
                  window=W if windowed else 0, sinks=K if windowed else 0, **kw)
    if sunk and not windowed:
        plain = _lean_twice(mli, dev, x, elem, f"{entry} W 0 K 0 {elem}", {counter: 1}, entry=entry, extra=(2, 2, 0, 0, extra[4]), H=2)
        assert_equal(got, plain, what=f"{entry} W {W} K {K}: the bits of W 0")
    if sunk and W == 1:
        z = kw["sink"].astype(np.float64)
        for b in rows:
            if case.lengths[b]:
                Kb, Vb = x.values_of(b)
                for h in range(2):
                    cols = slice(64 * h, 64 * h + 64)
                    newest = float(Kb[-1, cols].astype(np.float64) @ case.q[b, cols].astype(np.float64)) / 8.0
                    want = Vb[-1, cols].astype(np.float64) / (1.0 + np.exp(z[h] - newest))
                    # the condition scale of this head is |V[newest]| times the same factor
                    err = float(np.abs(got[b, cols] - want).max() / np.abs(want).max())
                    assert err <= tols["flat"], f"W 1: row {b} head {h} is {err:.3e} from the closed form"


# ---- the merge statistics against the launch's LDS -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _lds_case():
    return lc.SparseCase(5000, [519935], 519936, 16, families={0: "late_peak"})


# (entry point, arguments behind emb_dim)
LDS_ROWS = [("scan", ()), ("window", (1, 519935))]


@pytest.mark.parametrize("entry,extra", LDS_ROWS)
def test_statistics_fill_the_launch_lds(oracle, mli, dev, entry, extra):
    """(1, 519936, 16) at chunk_tokens 64: 8124 statistics pairs, 65024 bytes of dynamic LDS -- all a launch gets beside the
    kernels' static part; one page more is refused (REFUSALS).  The plain scan stages a pair per 64 tokens of n_sequence, the
    windowed one a pair per item of the span (W = S - 1: the whole row).  The row is judged on fp32 and bf16 pages."""
    case = _lds_case()
    try:
        _tune(mli, chunk_tokens=64)
        for elem in ("f32", "bf16"):
            x = _pages(case, elem, dev)
            want = {"scan_chunked": 1} if entry == "scan" else {"scan_heads_window": 1}
            got = _lean_twice(mli, dev, x, elem, f"S 519936 {entry} {elem}", want, entry=entry, extra=extra)
            _judge(oracle, x, got, [0], f"limits: S 519936, {entry}", elem, window=extra[1] if extra else 0)
    finally:
        _tune(mli, **DEFAULTS)


# ---- several heads: the widest rows ---------------------------------------------------------------------------------------------
HEADS_WIDE = [("f32", 512, 4), ("bf16", 1024, 8)]


@pytest.mark.parametrize("elem,D,H", HEADS_WIDE)
def test_heads_widest_rows(oracle, mli, dev, elem, D, H):
    """two 16-byte lane loads per row, the widest the multi-head scan takes: fp32 emb_dim 512, bf16 1024.  All rows judged."""
    x = _pages(_wide_case(D), elem, dev)
    got = _lean_twice(mli, dev, x, elem, f"heads D {D} {elem}", {"scan_heads_window": 1}, entry="heads", extra=(H,), H=H)
    _judge(oracle, x, got, list(range(8)), "limits: several heads, widest rows", elem, H=H)


@pytest.mark.parametrize("entry", ["alibi", "softcap", "sink_logits"])
@pytest.mark.parametrize("elem,D,H", HEADS_WIDE)
def test_heads_widest_rows_biased(oracle, mli, dev, elem, D, H, entry):
    """test_heads_widest_rows with the ALiBi bias, with the cap and with sink logits: the widest rows of their own kernel
    families ("scan_heads_alibi" / "scan_heads_softcap" / "scan_heads_sink_logits" counts the launch).  All rows judged.
    Sink logits: head size 128 at both lanes-per-head settings (fp32 32 lanes, bf16 16), two lane loads; the rows carry no
    score families (one logit per head serves every row).  A second launch puts +1e30 on the last head, which lies in the
    second lane load: exact zeros there on every non-empty row, the other heads' bits unchanged."""
    sunk = entry == "sink_logits"
    x = _pages(_wide_case(D, sunk), elem, dev)
    rows = list(range(8))
    extra, q, kw, counter = _biased(entry, x.case, H, H, 0, 0, dev, x=x, rows=rows)
    got = _lean_twice(mli, dev, x, elem, f"{entry} D {D} {elem}", {counter: 1}, entry=entry, extra=extra, H=H, q=q)
    _judge(oracle, x, got, rows, f"limits: several heads, widest rows, {entry}", elem, H=H, **kw)
    if sunk:
        import sink_logits_model as sl
        assert sl.second_lane_load(H - 1, H, D, lc.EPL[elem]) and not sl.second_lane_load(0, H, D, lc.EPL[elem])
        far = kw["sink"].copy()
        far[H - 1] = 1e30
        zeros = _lean_twice(mli, dev, x, elem, f"{entry} D {D} {elem}, +1e30 on head {H - 1}", {counter: 1}, entry=entry,
                            extra=extra[:4] + (_t(far, dev),), H=H)
        hd = D // H
        assert not zeros[:, (H - 1) * hd:].any(), "the +1e30 head is not exactly zero"
        assert_equal(zeros[:, :(H - 1) * hd], got[:, :(H - 1) * hd], what="the other heads under +1e30 on the last")
        _judge(oracle, x, zeros, rows, f"limits: several heads, widest rows, {entry}, +1e30", elem, H=H, sink=far)


# ---- standalone launchers ------------------------------------------------------------------------------------------------------
QKT_SHAPES = [("paged", "f32", 16360), ("paged", "bf16", 16360), ("naive", "f32", 15344)]


@pytest.mark.parametrize("form,elem,D", QKT_SHAPES)
def test_standalone_qkt_widest_rows(oracle, mli, dev, form, elem, D):
    """mli_qkt_paged[_bf16] and mli_qkt stage q in LDS: the widest rows that fit a launch's 64 KiB (emb_dim 16360 / 15344;
    four / one more are refused).  (2, 64, D), lengths 63 and 17; scores judged by f64_model.score_error, launched twice."""
    case = lc.SparseCase(5100 + D, [63, 17], 64, D)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    if form == "paged":
        x = _pages(case, elem, dev)
        call = lambda qkt: getattr(mli, "mli_qkt_paged" + ("_bf16" if elem == "bf16" else ""))(p(x.q), p(x.table), p(x.L), p(qkt), 2, 64, D, st)
        values_of = x.values_of
    else:
        kt, _ = case.dense()
        d_kt, d_q, d_L = _t(kt, dev), _t(case.q, dev), _t(case.lengths, dev)
        call = lambda qkt: mli.mli_qkt(p(d_q), p(d_kt), p(d_L), p(qkt), 2, 64, D, st)
        values_of = case.rows
    res = []
    for _ in range(2):
        qkt = torch.full((2, 64), lc.SENTINEL, device=dev)
        assert call(qkt) == 0
        res.append(host(qkt).copy())
    assert res[0].tobytes() == res[1].tobytes(), "second launch"
    for b in range(2):
        n = int(case.lengths[b])
        K, V = values_of(b)
        _, model, (xo, _, _) = lc.row_truth(oracle, case.q[b], K, V)[0]
        ck = Checker("flat", elem)
        ck.check(f"limits: standalone qkt {form}, D {D}", "scores", fm.score_error(res[0][b:b + 1, :n], model), fm.score_error(xo, model))
        ck.done()


SOFTMAX_V_SHAPES = [(24, 512, 64), (24, 512, 66)]


@pytest.mark.parametrize("B,S,D", SOFTMAX_V_SHAPES)
def test_softmax_v_vector_and_scalar_form(oracle, mli, dev, B, S, D):
    """mli_softmax_v reads V in float4 pieces where emb_dim is a multiple of 4 and element by element where it is not: both
    forms on the same lengths and probabilities (the float64 model's, rounded to fp32), several items per row, launched twice.
    Judged: every row, against sum p v in float64 with the fp32 oracle's softmax_v setting the tolerance."""
    from types import SimpleNamespace
    from accuracy_cases import edge_lengths
    L = edge_lengths(5200, B, S, (64, 256), top=S)
    rng = np.random.default_rng(5201 + D)
    q = (rng.random((B, 64), dtype=np.float32) * 2 - 1).astype(np.float32)
    kt = (rng.random((B, 64, S), dtype=np.float32) * 2 - 1).astype(np.float32)
    v = (rng.random((B, S, D), dtype=np.float32) * 2 - 1).astype(np.float32)
    probs = fm.softmax(fm.scores(q, kt, L), L).astype(np.float32)
    v[np.arange(S)[None, :] >= L[:, None]] = 1e30                       # dead slots: finite and gross
    model = SimpleNamespace(lengths=L.astype(np.int64), o=fm.attend(probs, v, L), o_scale=fm.attend_abs(probs, v, L).max(axis=1))
    o_oracle = np.zeros((B, D), np.float32)
    oracle.softmax_v_host(probs, v, o_oracle, L)
    d_p, d_v, d_L = _t(probs, dev), _t(v, dev), _t(L, dev)
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    ws[:lc.COUNTER_BYTES] = 0
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    res = []
    try:
        _tune(mli, chunk_tokens=64)
        for _ in range(2):
            out = torch.full((B, D), lc.SENTINEL, device=dev)
            assert mli.mli_softmax_v(p(d_p), p(d_v), p(d_L), p(out), B, S, D, p(ws), need,
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
            res.append(host(out).copy())
    finally:
        _tune(mli, **DEFAULTS)
    assert res[0].tobytes() == res[1].tobytes(), "second launch"
    _counters_are_zero(ws, "softmax_v")
    ck = Checker("flat", "f32")
    ck.check(f"limits: standalone softmax_v, D {D}", "attention", fm.attention_error(res[0], model), fm.attention_error(o_oracle, model))
    ck.done()


# ---- the causal prompt scan ----------------------------------------------------------------------------------------------------
def _prompt_twice(dev, x, segs, qv, elem, H, Hkv, W, K, cap, what, sink=None):
    """mli_prompt_scan_paged[_softcap / _sink_logits] twice: the same bits, one launch of the family each, nothing else;
    [n_q, D] on the host"""
    from min_llm_inference_amd import ops
    c = x.case
    q_dev = _t(qv, dev)
    z_dev = None if sink is None else _t(np.asarray(sink, np.float32), dev)
    ops.reset_launch_counts()
    res = []
    for _ in range(2):
        out = torch.full(qv.shape, lc.SENTINEL, device=dev)
        ops.prompt_scan_paged(q_dev, x.table, segs, out, c.B, c.S, lc.ELEM[elem], n_heads=H, n_kv_heads=Hkv, window=W, sinks=K, softcap=cap,
                              sink_logits=z_dev)
        res.append(host(out).copy())
    assert_equal(res[1], res[0], what=f"{what}: second launch")
    want = {f: 0 for f in SCAN_FAMILIES}
    want["scan_prompt_sink_logits" if sink is not None else "scan_prompt" if cap is None else "scan_prompt_softcap"] = 2
    assert _counts() == want, f"{what}: launch counters {_counts()}"
    assert np.isfinite(res[0]).all() and (res[0] != lc.SENTINEL).any(axis=1).all(), what
    return res[0]


def _prompt_judged(oracle, dev, x, segs, elem, H, Hkv, W, K, what, cap=None, q_rows=None, sunk=False):
    """sunk: with sink logits learned per head from the queries themselves (limit_cases.learned_sparse over what the pages hold,
    the condition on them asserted); all -inf then gives the bits of the plain launch"""
    rows, pos = pm.queries(segs)
    qv = pm.query_vectors(x.case.q if q_rows is None else q_rows, rows, pos)
    z = None
    if sunk:
        import sink_logits_model as sl
        lse = lc.judged_lse(x.case, x.values_of, rows, H, Hkv, *_mask(x.case.S, W, K), q=qv, lengths=pos + 1)
        z = lc.learned_sparse(lse)
        print(f"SINK_LOGITS {what}: logits {[round(float(t), 2) for t in z]}; share in the band on {lc.biting(lse, z, what):.2f} of the judged pairs")
    got = _prompt_twice(dev, x, segs, qv, elem, H, Hkv, W, K, cap, what, sink=z)
    truth = pm.long_truth(oracle, x.case, x.values_of, qv, rows, pos, H, Hkv, W, K, cap=cap, sink=z)
    res = pm.long_compare(got, truth, what=what)
    pm.hm.assert_within(res, what)
    if sunk:
        SINK_RATIOS.extend(worst / tol for _, worst, tol in res)
        plain = _prompt_twice(dev, x, segs, qv, elem, H, Hkv, W, K, None, what + " plain")
        assert np.abs(got - plain).max() > 1e-3, f"{what}: the logits change nothing"
        assert_equal(_prompt_twice(dev, x, segs, qv, elem, H, Hkv, W, K, None, what + " all -inf", sink=sl.none(H)), plain,
                     what=f"{what}: all -inf against the plain launch")
    return got


PROMPT_WIDE = [("f32", 512), ("bf16", 1024)]


@pytest.mark.parametrize("elem,D", PROMPT_WIDE)
def test_prompt_scan_widest_rows(oracle, mli, dev, elem, D):
    """One head at (4, 128, D) with two 16-byte lane loads per row, the widest the prompt scan takes (fp32 emb_dim 512, bf16
    1024; 516 / 1032 and fp8 pages are refused: REFUSALS), plain and under W 40 with 4 sinks.  Every query judged; "scan_prompt"
    counts the launch."""
    from min_llm_inference_amd import ops
    tq = ops.prompt_scan_tq(D, 1, lc.ELEM[elem])
    case = lc.SparseCase(5300 + D, [128, 100, 64, 17], 128, D, families={0: "late_peak", 1: "early_peak"}, full_rows=True)
    x = _pages(case, elem, dev)
    segs = [(1, 90, 10), (0, 128 - (tq + 1), tq + 1), (3, 15, 2), (2, 0, 2 * tq + 1)]
    for W, K in ((0, 0), (40, 4)):
        _prompt_judged(oracle, dev, x, segs, elem, 1, 1, W, K, f"limits: prompt scan, widest rows, D {D} {elem} W {W} K {K}")
    # the same width with several heads and sink logits (the single-head kernels have none): fp32 D 512 H 4, bf16 D 1024 H 8 on
    # 2, head size 128; rows without score families, one logit per head serving every query; "scan_prompt_sink_logits" counts
    H, Hkv = (4, 4) if elem == "f32" else (8, 2)
    flat = lc.SparseCase(5300 + D, [128, 100, 64, 17], 128, D, full_rows=True)
    x = _pages(flat, elem, dev)
    for W, K in ((0, 0), (40, 4)):
        _prompt_judged(oracle, dev, x, segs, elem, H, Hkv, W, K, f"limits: prompt scan, widest rows, sink logits, D {D} H {H}/{Hkv} {elem} W {W} K {K}",
                       sunk=True)


PROMPT_ROWS = [(1, None), (2, None), (2, CAP), (2, "sink_logits")]


@pytest.mark.parametrize("elem", ["f32", "bf16"])
@pytest.mark.parametrize("H,cap", PROMPT_ROWS)
def test_prompt_scan_on_the_last_row(oracle, mli, dev, H, cap, elem):
    """n_batch 16384, the last the prompt scan takes (16385 is refused: REFUSALS), with segments on rows 0, 8191 and 16383 and
    on a short row, one head and two, and two heads under the cap.  Every query judged; "scan_prompt" / "scan_prompt_softcap"
    counts the launch."""
    from min_llm_inference_amd import ops
    D = 64 * H
    case, _ = _heads_case(D)
    x = _pages(case, elem, dev)
    tq = ops.prompt_scan_tq(D, H, lc.ELEM[elem])
    segs = [(16383, 62 - tq, tq + 1), (7, 30, 3), (0, 0, 2 * tq + 1), (8191, 40, tq)]
    if cap == "sink_logits":        # two heads with sink logits: "scan_prompt_sink_logits" counts the launch
        _prompt_judged(oracle, dev, x, segs, elem, H, H, 0, 0, f"limits: prompt scan, B 16384, H {H} sink logits {elem}", sunk=True)
        return
    _prompt_judged(oracle, dev, x, segs, elem, H, H, 0, 0, f"limits: prompt scan, B 16384, H {H} cap {cap} {elem}", cap=cap,
                   q_rows=None if cap is None else _scaled_q(case, H, H))


@functools.lru_cache(maxsize=1)
def _hand_off_case(D):
    return lc.SparseCase(5400, [64, 40, 17, 64], 64, D, families={0: "early_peak"}, full_rows=True)


PROMPT_WINDOWS = [(63, True), (64, False)]


@pytest.mark.parametrize("W,windowed", PROMPT_WINDOWS)
@pytest.mark.parametrize("elem,H", [("f32", 1), ("bf16", 1), ("f32", 2)])
def test_prompt_window_hand_off(oracle, mli, dev, elem, H, W, windowed):
    """(4, 64, 64): W 63 is the last window the prompt scan masks by -- only the query at position 63 drops slot 0, which on
    row 0 carries an early peak -- and W 64 is the plain mask: the bits of W 0.  Every query judged."""
    x = _pages(_hand_off_case(64), elem, dev)
    segs = [(3, 0, 64), (1, 33, 7), (0, 56, 8)]
    what = f"limits: prompt scan, hand-off W {W} H {H} {elem}"
    got = _prompt_judged(oracle, dev, x, segs, elem, H, H, W, 0, what)
    rows, pos = pm.queries(segs)
    plain = _prompt_twice(dev, x, segs, pm.query_vectors(x.case.q, rows, pos), elem, H, H, 0, 0, None, what + " plain")
    differs = (got != plain).any(axis=1)
    if windowed:
        assert differs[pos == 63].all(), "the queries at position 63 drop slot 0"
    else:
        assert not differs.any(), "W = n_sequence is the plain mask"


@functools.lru_cache(maxsize=1)
def _x_pages(elem, dev, B=16, S=4096, D=64):
    """pages of (16, 4096, 64) with x, K and V random in [-1, 1) on the device, every row whole, pages in shuffled order"""
    gen = torch.Generator(device=dev).manual_seed(5500)
    pool = torch.rand((B * S // 16, 16, 3, D), generator=gen, device=dev) * 2 - 1
    pool = pool if elem == "f32" else pool.to(torch.bfloat16)
    order = np.random.default_rng(5501).permutation(B * S // 16).reshape(B, S // 16)
    table = _t(pool.data_ptr() + order.astype(np.int64) * (16 * 3 * D * lc.ESIZE[elem]), dev)
    return pool, order, table


def _slots(pool, order, rows, pos):
    """float32 [n, 3, D]: x, K, V of the (row, position) pairs as the pages hold them"""
    pages = torch.from_numpy(order[np.asarray(rows), np.asarray(pos) // 16]).to(pool.device)
    return pool[pages, torch.from_numpy(np.asarray(pos) % 16).to(pool.device)].float().cpu().numpy()


PROJECT_ELEMS = ["f32", "bf16"]


@pytest.mark.parametrize("elem", PROJECT_ELEMS)
def test_prompt_project_q_at_the_last_segment(mli, dev, elem):
    """mli_prompt_project_q with 65535 segments of one position, the last count it takes (the gather's grid has a segment per
    y; 65536 are refused: REFUSALS), over (16, 4096, 64), offsets in reversed order.  q of segments 0, 32767, 65534 and a fixed
    sample of 64 against float64 x . Wq at the fp32 chain's own bound D 2^-24 sum |x w|; every q row finite;
    "gemm_f32_rows64" / "gemm_bf16_widened" counts the product."""
    from helpers import bf16_round
    from min_llm_inference_amd import ops
    B, S, D, n = 16, 4096, 64, 65535
    pool, order, table = _x_pages(elem, dev)
    i = np.arange(n, dtype=np.int64)
    rows, first, offs = (i * 7) % B, (i * 2654435761) % S, n - 1 - i
    w = ((np.random.default_rng(5502).random((D, D), dtype=np.float32) * 2 - 1) / np.sqrt(D)).astype(np.float32)
    w = w if elem == "f32" else bf16_round(w)
    wq = _t(w, dev).to(torch.float32 if elem == "f32" else torch.bfloat16)
    arrays = [_t(a.astype(np.int32), dev) for a in (rows, first, np.ones(n, np.int64), offs)]
    gathered = torch.empty(n * D, dtype=torch.float32, device=dev)
    q = torch.full((n, D), lc.SENTINEL, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    ops.reset_launch_counts()
    rc = mli.mli_prompt_project_q(p(table), *map(p, arrays), p(wq), p(gathered), p(q), n, 1, n, B, S, D, lc.ELEM[elem],
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    family = "gemm_f32_rows64" if elem == "f32" else "gemm_bf16_widened"
    assert ops.launch_count(family) == 1 and not any(_counts().values())
    got = host(q)
    assert np.isfinite(got).all() and (got != lc.SENTINEL).any(axis=1).all()
    judged = lc.sample_rows(n, [0, 32767, 65534])
    xs = _slots(pool, order, rows[judged], first[judged])[:, 0].astype(np.float64)
    exact = xs @ w.astype(np.float64)
    bound = D * 2.0 ** -24 * (np.abs(xs) @ np.abs(w).astype(np.float64))
    worst = float((np.abs(got[offs[judged]].astype(np.float64) - exact) / bound).max())
    print(f"PROJECT Q 65535 segments {elem}: worst error {worst:.3e} of the bound D 2^-24 sum |x w|")
    assert worst <= 1.0


def test_offsets_beyond_2_31_prompt_logits(oracle, mli, dev):
    """mli_paged_prompt_logprobs with n_positions 16384 and n_vocab 131072 at emb_dim 64: the logits inside the scratch are 2^31
    floats (8 GiB), so the rows of the last positions lie beyond 2^31 elements.  Four whole rows of (16, 4096, 64) are scored.
    Judged: the last eight positions -- prompt_model.compare_given against the float64 forward of those positions over what
    the pages hold (projection, causal softmax over the row, logits), at compare_given's own tolerance; the position at
    n_sequence - 1 reports -inf.
    "scan_prompt" counts the scan.  Skips when less than twice the scratch is free."""
    from min_llm_inference_amd import ops
    B, S, D, V = 16, 4096, 64, 131072
    need = int(mli.mli_prompt_logprobs_scratch_bytes(4 * S, D, V))
    assert need > 8 << 30
    _WS.clear()
    torch.cuda.empty_cache()
    _needs(dev, need, "the scratch of 16384 positions x 131072 tokens")
    pool, order, table = _x_pages("f32", dev)
    rng = np.random.default_rng(5600)
    emb = _t((rng.standard_normal((V, D)) * 0.5).astype(np.float32), dev)
    inp = rng.integers(0, V, size=(B, S)).astype(np.int32)
    wq = _t((rng.standard_normal((D, D)) * (2.0 / np.sqrt(D))).astype(np.float32), dev)
    segs = [(3, 0, S), (9, 0, S), (0, 0, S), (15, 0, S)]
    ops.reset_launch_counts()
    got = host(ops.paged_prompt_logprobs(table, _t(inp, dev), wq, emb, segs, B, S, lc.ELEM["f32"])[0]).copy()
    assert ops.launch_count("scan_prompt") == 1 and ops.launch_count("scan_prompt_softcap") == 0
    ends = np.arange(len(got)) % S == S - 1                 # the position at n_sequence - 1 of every row has no next token
    assert not np.isnan(got).any() and (got[~ends] > -np.inf).all() and (got[ends] == -np.inf).all()
    # the float64 forward of the last eight positions of row 15, from what the pages hold: q = x . Wq, the causal softmax over
    # the row's first t + 1 tokens, attention . emb^T -- nothing of it is a kernel's output
    slots = _slots(pool, order, np.full(S, 15), np.arange(S)).astype(np.float64)          # [S, 3, D]: x, K, V
    x64, K64, V64 = slots[:, 0], slots[:, 1], slots[:, 2]
    w64, e64 = host(wq).astype(np.float64), host(emb).astype(np.float64)
    logits = np.zeros((8, V))
    for i, t in enumerate(range(S - 8, S)):
        score = K64[:t + 1] @ (x64[t] @ w64) / np.sqrt(D)
        prob = np.exp(score - score.max())
        logits[i] = ((prob / prob.sum()) @ V64[:t + 1]) @ e64.T
    given = np.asarray([inp[15, t + 1] if t + 1 < S else -1 for t in range(S - 8, S)], np.int64)
    zero = np.zeros((8, 0))
    err, tol, bad = pm.compare_given((got[-8:], zero, zero), logits.astype(np.float32), given, 0)
    print(f"PROMPT LOGITS beyond 2^31: worst error {err:.3e}, bound {tol:.3e}")
    assert not bad and err <= tol, (err, tol, bad)
    torch.cuda.empty_cache()


def test_rope_at_the_smallest_head_size(oracle, mli, dev):
    """head size 2 (emb_dim 64, 32 heads: one pair per head), the near side of rope_half's rule; 17 and 33 are refused
    (REFUSALS).  tests/test_rope_gemm_gpu.py's whole check of the decode projection; "gemm_f32_rope" counts the launch."""
    from test_rope_gemm_gpu import R64, _check, _latest_case
    _check(oracle, mli, dev, "limits: head size 2", _latest_case(5700, "f32", 70, 64, 64), "latest", 32, R64, ())


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(mli, dev):
    """Every refusal of the table on the device: MLI_ERR_BAD_ARG, no launch counted, the workspace's counters untouched.  (The
    same calls return the same status without a GPU -- tests/test_shape_limits_cpu.py -- so no pointer is ever followed.)"""
    from min_llm_inference_amd import ops
    ws = torch.zeros(16 << 20, dtype=torch.uint8, device=dev)
    ops.reset_launch_counts()
    try:
        for entry, args, limit, ct in lc.REFUSALS:
            _tune(mli, chunk_tokens=ct)
            rc = lc.call_refusal(mli, entry, args, workspace=ws.data_ptr(), workspace_bytes=ws.numel(),
                                 stream=torch.cuda.current_stream().cuda_stream)
            assert rc == lc.BAD_ARG, (entry, args, limit, rc)
    finally:
        _tune(mli, **DEFAULTS)
    assert not any(_counts().values()), _counts()
    assert not any(ops.launch_count(f) for f in OTHER_FAMILIES), {f: ops.launch_count(f) for f in OTHER_FAMILIES}
    assert not host(ws).any()
