"""The scratch contract of include/mli_kernels.h, held with fenced, poisoned buffers (tests/scratch_fence.py).

Every case runs one entry point at the smallest shape that reaches the plan named, with everything the call touches
carved from one arena -- inputs, pages, outputs, workspace, decoder scratch, logprob arrays -- and asserts:
  a. exactly the public size function's bytes are enough (status 0) under every knob setting of the case;
  b. every guard byte of the arena is intact;
  c. the outputs are bit-identical with the scratch body zero, 0xFF (NaN / -1), and left behind by a DIFFERENT call (another
     shape, another score family; a multi-head call before a plain one and the reverse); the counter region is zeroed
     once, at allocation;
  d. the whole 64 KiB counter region, the ticket included, is zero after every call; nothing is non-finite, no output
     sentinel survives on a live row, rows of length 0 are exact zeros;
  e. once per case the result is within f64_model.tolerance (of the fp32 oracle's own error) of the float64 model, so
     that "the same bits" cannot mean "the same wrong bits";
  f. scan-only and decoder entry points, called with a valid pointer and 0, 65536, 65536 + the statistics region,
     need - 256 and need bytes, either refuse (negative status, not one byte of the arena changed) or succeed with the
     fence directly behind the bytes given (guards intact, the bits of the full-size run).
The high-water mark of every scratch case (last byte of the 0xFF body the call wrote, over the size asked for) is
recorded; MLI_SCRATCH_REPORT=<file> writes the table.  The compositions (fill or attention first, then the scan or the
head) are fenced but not laddered: what they answer to need - 256 bytes is recorded.  The entry points without scratch
assert b, d and e on fenced outputs."""
import contextlib
import ctypes
import os

import numpy as np
import pytest
import torch

import f64_model as fm
import gemm_model as gm
import gqa_model as gqa
import alibi_model as alm
import logprobs_model as lpm
import prompt_model as pm
import softcap_model as scm
import sampling_cases
import scratch_fence as sf
from accuracy_cases import apply_family, base_case, oracle_scan, poison_contiguous
from accuracy_gpu import pages_on_device
from helpers import PAGE, bf16_bits, build_page_pool, paged_case

pytestmark = pytest.mark.gpu

ELEM = {"f32": 0, "bf16": 1, "fp8": 2}
ESIZE = {"f32": 4, "bf16": 2, "fp8": 1}
SENTINEL = 12345.0
ISENTINEL = -77
COUNTERS = sf.COUNTER_BYTES
TABLE = {}        # case -> (high-water mark in bytes, bytes asked for)
REFUSALS = {}     # fill-first composition -> status with need - 256 bytes (recorded, not asserted)


@pytest.fixture(scope="module", autouse=True)
def _report():
    TABLE.clear()
    REFUSALS.clear()
    yield
    path = os.environ.get("MLI_SCRATCH_REPORT")
    if path and TABLE:
        with open(path, "w") as f:
            f.write("| case | high water | need | high water / need |\n|---|---:|---:|---:|\n")
            for what, (high, need) in TABLE.items():
                f.write(f"| {what} | {high} | {need} | {high / need if need else 0.0:.3f} |\n")
            for what, rc in REFUSALS.items():
                f.write(f"refusal | {what} | status {rc}\n")


# ---- knobs: every one is put back ------------------------------------------------------------------------------------------
# The library has no getter, so a knob is put back to the value knobs() last set, or to the default mli_kernels.h states for
# it (the mli_tune comment); test_the_knob_defaults_are_the_headers holds this copy to the header's text.
DEFAULTS = {"chunk_tokens": 0, "scan_merge": 1, "scan_stream": 1, "scan_stream_min_tokens": 1 << 21,
            "scan_stream_dynamic_pct": 4, "scan_stream_granule": 64, "fused_softmax": -1, "gemm_panel": 1,
            "gemm_tall_tiles": 1}
_current = {}


@contextlib.contextmanager
def knobs(mli, **kw):
    before = {k: _current.get(k, DEFAULTS[k]) for k in kw}
    try:
        for k, v in kw.items():
            assert mli.mli_tune(k.encode(), v) == 0, (k, v)
            _current[k] = v
        yield
    finally:
        for k, v in before.items():
            mli.mli_tune(k.encode(), v)
            _current[k] = v


HEADER_SAYS = {   # what the mli_tune comment of include/mli_kernels.h says of each default, as a pattern over its text
    "chunk_tokens": r'"chunk_tokens"\s+{v} = heuristic',
    "scan_merge": r'"scan_merge"\s+\(lean mode\) {v} \(default\)',
    "scan_stream": r'"scan_stream"\s+\(lean mode\) {v} \(default\)',
    "scan_stream_min_tokens": r'n_batch \* n_sequence >= 2\^{log2}',
    "scan_stream_dynamic_pct": r'per cent \(default {v},',
    "scan_stream_granule": r'many pages \(default {v},',
    "fused_softmax": r'{v} \(default\) =\s+\*?\s*fuse when',
    "gemm_panel": r'"gemm_panel"\s+{v} \(default\)',
    "gemm_tall_tiles": r'"gemm_tall_tiles"\s+{v} \(default\)',
}


def test_the_knob_defaults_are_the_headers():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "mli_kernels.h")) as f:
        text = f.read()
    assert set(HEADER_SAYS) == set(DEFAULTS)
    for key, value in DEFAULTS.items():
        pat = HEADER_SAYS[key].format(v=value, log2=value.bit_length() - 1)
        assert re.search(pat, text), f"mli_kernels.h does not state {value} as the default of {key!r} ({pat})"


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def launches(mli, family):
    n = ctypes.c_ulonglong(0)
    assert mli.mli_launch_count(family.encode(), ctypes.byref(n)) == 0
    return int(n.value)


def stats_bytes(B, S, H=1):
    """The statistics region behind the counters (the header's layout: one float2 per row, 64 tokens and head, 256-byte
    aligned)."""
    return (B * -(-S // 64) * H * 8 + 255) // 256 * 256


def length_vectors(seed, B, S):
    """Lengths that always include 0, 1, 63, 64, 65, S - 1 and S: one vector where the batch has the rows, several where it
    has not.  (accuracy_cases.edge_lengths forces eleven edges and two long rows in, thirteen rows at least; the shapes
    here have twelve, six and four.)"""
    edges = sorted({0, 1, 63, 64, 65, S - 1, S})
    rng = np.random.default_rng(seed)
    out = []
    for i in range(0, len(edges), B):
        part = edges[i:i + B]
        L = rng.integers(2, S + 1, size=B)
        L[:len(part)] = part
        out.append(L.astype(np.int32))
    return out


def f32(raw, shape):
    return raw.view(np.float32).reshape(shape)


def check_rows(out, L, what):
    """d: nothing non-finite, no sentinel on a live row, rows of length 0 exact zeros."""
    assert np.isfinite(out).all(), f"{what}: non-finite value"
    L = np.asarray(L)
    assert not out[L == 0].any(), f"{what}: a row of length 0 is not zero"
    assert not (out[L > 0] == SENTINEL).any(), f"{what}: the sentinel survives on a live row"


# ---- a paged scan problem ----------------------------------------------------------------------------------------------------
class Paged:
    """q, lengths and the pages of a case in a score family (an assignment of families for several heads), the float64
    model and the fp32 oracle of what the pages hold.  place() carves all of it from an arena."""

    def __init__(self, oracle, dev, seed, B, S, D, elem, family, lengths, H=1, Hkv=1, W=0, K=0, slopes=None, cap=None):
        """slopes [H] float32: the ALiBi call; cap: the soft-capped call, q scaled by softcap_model.scale_q's rule"""
        self.B, self.S, self.D, self.elem, self.H, self.Hkv, self.W, self.K = B, S, D, elem, H, Hkv, W, K
        self.slopes, self.cap = slopes, cap
        c = base_case(seed, B, S, D, lengths)
        if H == 1:
            q, kt = apply_family(c, family)
            self.fams = (family,)
        else:
            q, kt = gqa.apply_gqa_families(c, H, Hkv, family)
            self.fams = gqa.head_families(family, H, Hkv)
        if cap is not None:
            q = scm.scale_q(q, kt, c["lengths"], H, Hkv)
        self.q, self.L, self.table = q, c["lengths"], c["table"]
        self.pool, values = pages_on_device(oracle, dev, c, q, kt, c["v_cache"], elem, "nan")
        self.k_rows = fm.gather_pages(values, self.table, self.L, S, D, 1)
        self.v_rows = fm.gather_pages(values, self.table, self.L, S, D, 2)
        self.ktm = self.k_rows.transpose(0, 2, 1)
        self.oracle = oracle

    def room(self, qkt=False):
        B, S, D = self.B, self.S, self.D
        return [self.q.nbytes, self.L.nbytes, self.pool.numel() * self.pool.element_size(), self.table.size * 8, B * D * 4] + \
               ([B * S * 4] if qkt else []) + ([self.slopes.nbytes] if self.slopes is not None else [])

    def place(self, arena, p="", qkt=False):
        arena.carve_from(p + "q", self.q)
        arena.carve_from(p + "lengths", self.L)
        place_pool(arena, self.pool, self.table, self.elem, p)
        if self.slopes is not None:
            arena.carve_from(p + "slopes", self.slopes)
        arena.carve(p + "out", self.B * self.D * 4)
        arena.view(p + "out", torch.float32).fill_(SENTINEL)
        if qkt:
            arena.carve(p + "qkt", self.B * self.S * 4)
            arena.view(p + "qkt", torch.float32).fill_(SENTINEL)

    def scan(self, mli, arena, p, entry, n, phases=7):
        a = lambda name: arena.ptr(p + name)
        B, S, D, e = self.B, self.S, self.D, ELEM[self.elem]
        front, tail = (a("q"), a("table"), a("lengths")), (arena.ptr("ws"), n, stream())
        if entry == "plain":
            return mli.mli_decode_scan_paged(*front, a("qkt") if phases < 4 else None, a("out"), B, S, D, e, phases, *tail)
        if entry == "heads":
            return mli.mli_decode_scan_paged_heads(*front, a("out"), B, S, D, self.H, e, *tail)
        if entry == "window":
            return mli.mli_decode_scan_paged_window(*front, a("out"), B, S, D, self.H, self.W, e, *tail)
        if entry == "sinks":
            return mli.mli_decode_scan_paged_sinks(*front, a("out"), B, S, D, self.H, self.W, self.K, e, *tail)
        if entry == "alibi":
            return mli.mli_decode_scan_paged_alibi(*front, a("out"), B, S, D, self.H, self.Hkv, self.W, self.K, a("slopes"), e, *tail)
        if entry == "softcap":
            return mli.mli_decode_scan_paged_softcap(*front, a("out"), B, S, D, self.H, self.Hkv, self.W, self.K, self.cap, e, *tail)
        assert entry == "gqa", entry
        return mli.mli_decode_scan_paged_gqa(*front, a("out"), B, S, D, self.H, self.Hkv, self.W, self.K, e, *tail)

    def judge(self, out, what, H=None, Hkv=None, W=None, K=None):
        """e: attention_result against the float64 model, tolerance from the fp32 oracle's own error."""
        H, Hkv = self.H if H is None else H, self.Hkv if Hkv is None else Hkv
        W, K = self.W if W is None else W, self.K if K is None else K
        if H > 1 and (self.slopes is not None or self.cap is not None):      # the derived bound of alibi_model / softcap_model
            m, arg = (alm, self.slopes) if self.slopes is not None else (scm, self.cap)
            model = (m.AlibiModel if m is alm else m.SoftcapModel)(self.q, self.ktm, self.v_rows, self.L, H, Hkv, arg, W, K)
            worst, tol = m.compare(out, m.eval_fp32(self.q, self.ktm, self.v_rows, self.L, H, Hkv, arg, W, K), model, what=what)
            assert worst <= tol, f"{what}: {worst:.3e} > tol {tol:.3e}"
            return
        model = gqa.model_gqa(self.q, self.ktm, self.v_rows, self.L, H, Hkv, W, K)
        o_or = gqa.oracle_gqa(self.oracle, self.q, self.ktm, self.v_rows, self.L, H, Hkv, W, K)
        fams = self.fams if H == self.H else (self.fams[0],) * H
        gqa.assert_within(gqa.compare(out, o_or, model, fams, what=what), what)

    def judge_probabilities(self, p, what):
        model = fm.Model(self.q, self.ktm, self.v_rows, self.L)
        _, p_or, _ = oracle_scan(self.oracle, self.q, self.ktm, self.v_rows, self.L)
        err, e_or = fm.probability_error(p, model), fm.probability_error(p_or, model)
        tol = fm.tolerance(e_or)
        print(f"SCRATCH {what} | probabilities: kernel {err.max():.3e}  oracle {e_or.max():.3e}  tol {tol:.3e}")
        assert err.max() <= tol, f"{what}: probabilities {err.max():.3e} > tol {tol:.3e}"


def heads_need(mli, pb):
    n = int(mli.mli_attention_heads_workspace_bytes(pb.B, pb.S, pb.D, pb.H))
    assert n > 0
    return n


@pytest.fixture(scope="module")
def others(oracle, mli, dev):
    """The different calls that use a case's scratch before its "keep" run: another shape, another score family; several
    heads for a plain case, one head for the rest.  Always several items per row, so that they leave partial rows and
    statistics behind."""
    rng = np.random.default_rng(900)
    L = rng.integers(1, 193, size=7).astype(np.int32)
    L[:3] = [192, 130, 0]
    return {"heads": Paged(oracle, dev, 901, 7, 192, 128, "f32", "mixed", L, H=2, Hkv=2),
            "plain": Paged(oracle, dev, 902, 7, 192, 64, "f32", "peaked", L)}


def other_call(mli, arena, other, need):
    """The other call on the case's workspace, told its own size (the fence moves with it), checked like every call."""
    entry = "heads" if other.H > 1 else "plain"
    n = heads_need(mli, other)

    def run():
        arena.resize("ws", n)
        with knobs(mli, chunk_tokens=64):
            rc = other.scan(mli, arena, "o.", entry, n)
        arena.assert_guards_intact("the other call")
        got = f32(sf.bits(arena.view("o.out")), (other.B, other.D))
        check_rows(got, other.L, "the other call")
        arena.resize("ws", need)
        return rc
    return run


def contract(arena, what, call, images, outputs, need, other=None, counters=COUNTERS, scratch="ws", ladder=False,
             ladder_all_ok=False, stats=0):
    """a - d and f of the module docstring for one call(bytes) -> status; returns the bits of the outputs."""
    first, high = sf.run_under_fills(arena, scratch, lambda: call(need), images, outputs, other, counters, what)
    TABLE[what] = (high, need)
    print(f"SCRATCH {what} | high water {high} of {need} bytes")
    if ladder:
        sizes = [n for n in (0, COUNTERS, COUNTERS + stats, need - 256, need) if 0 <= n <= need]
        rungs = sf.run_ladder(arena, scratch, sizes, call, images, outputs, first, counters, what)
        print(f"SCRATCH {what} | ladder {rungs}")
        assert rungs[-1] == (need, 0), rungs
        if ladder_all_ok:
            assert all(rc == 0 for _, rc in rungs), f"{what}: a plan without a body refused a size: {rungs}"
        arena.resize(scratch, need)
    return first


def scan_case(mli, dev, pb, other, what, entry, need, phases=7, ladder_all_ok=False):
    """A scan problem and the other call's in one arena, the workspace behind them; runs the contract and returns
    (arena, attention_result, probabilities or None)."""
    qkt = phases < 4
    n_other = heads_need(mli, other)
    arena = sf.Arena(sf.Arena.room(*pb.room(qkt), *other.room(), max(need, n_other)), dev)
    pb.place(arena, "", qkt)
    carve_workspace(arena, other, need, n_other)
    outputs = ["out"] + (["qkt"] if qkt else [])
    first = contract(arena, what, lambda n: pb.scan(mli, arena, "", entry, n, phases), sf.save(arena, outputs), outputs, need,
                     other=other_call(mli, arena, other, need), ladder=True, ladder_all_ok=ladder_all_ok,
                     stats=stats_bytes(pb.B, pb.S, pb.H))
    out = f32(first["out"], (pb.B, pb.D))
    check_rows(out, pb.L, what)
    probs = f32(first["qkt"], (pb.B, pb.S)) if qkt else None
    if qkt:
        assert np.isfinite(probs).all() and not (probs == SENTINEL).any(), f"{what}: qkt_output"
    return arena, out, probs


# ---- mli_decode_scan_paged, phases 3 and 7 -----------------------------------------------------------------------------------------
SETTINGS = {"c64": ({"chunk_tokens": 64}, "flat"), "c64-combine": ({"chunk_tokens": 64, "scan_merge": 0}, "late_peak"),
            "c1024": ({"chunk_tokens": 1024}, "offset-")}


def _scan_grid():
    out = []
    for elem in ("f32", "bf16"):
        for phases in (3, 7):
            for setting in SETTINGS:
                if not (phases == 3 and setting == "c64-combine"):      # the materialising form always combines
                    out.append((12, 256, 64, elem, phases, setting))
    out += [(12, 256, 64, "fp8", 7, s) for s in SETTINGS]
    out += [(4, 256, 2048, "f32", p, "c64") for p in (3, 7)]            # the D-split: rows split across the four waves
    out += [(6, 256, 1024, "bf16", p, "c64") for p in (3, 7)]           # two lane loads
    out += [(12, 256, 512, "fp8", 7, "c64"), (12, 256, 1024, "fp8", 7, "c64")]   # one token slot per load; two lane loads
    return out


@pytest.mark.parametrize("B,S,D,elem,phases,setting", _scan_grid(), ids=lambda v: str(v))
def test_decode_scan_paged(oracle, mli, dev, others, B, S, D, elem, phases, setting):
    kn, family = SETTINGS[setting]
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    assert need > COUNTERS
    for i, L in enumerate(length_vectors(1000 + D + phases, B, S)):
        what = f"decode_scan_paged phases {phases} {elem} ({B}, {S}, {D}) {setting}" + (f" lengths {i}" if i else "")
        pb = Paged(oracle, dev, 1100 + D + i, B, S, D, elem, family, L)
        with knobs(mli, **kn):
            assert mli.mli_launch_counts_reset() == 0
            _, out, probs = scan_case(mli, dev, pb, others["heads"], what, "plain", need, phases,
                                      ladder_all_ok=setting == "c1024")
            assert launches(mli, "scan_equal_shares") == 0 and launches(mli, "scan_chunked") > 0
        pb.judge(out, what)
        if probs is not None:
            pb.judge_probabilities(probs, what)


# ---- the equal-shares scan -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [(4, 64), (12, 16)], ids=lambda v: f"dyn{v[0]}-gran{v[1]}")
@pytest.mark.parametrize("elem", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("S", [1024, 256])
def test_equal_shares_scan(oracle, mli, dev, others, S, elem, split):
    """n_sequence 1024 is the shortest the equal-shares scan takes: there it must run and not hand back.  At 256 the same
    settings hand the call to the chunked scan, which shows as that kernel's count; the contract holds either way."""
    B, D = 12, 64
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    L = length_vectors(1200 + S, B, S)[0]
    what = f"equal shares {elem} ({B}, {S}, {D}) dyn {split[0]} granule {split[1]}"
    pb = Paged(oracle, dev, 1300 + S, B, S, D, elem, "early_peak", L)
    with knobs(mli, scan_stream_min_tokens=0, scan_stream_dynamic_pct=split[0], scan_stream_granule=split[1]):
        assert mli.mli_launch_counts_reset() == 0
        _, out, _ = scan_case(mli, dev, pb, others["heads"], what, "plain", need)
        ran, chunked = launches(mli, "scan_equal_shares"), launches(mli, "scan_chunked")
    print(f"SCRATCH {what} | launches: equal shares {ran}, chunked {chunked}")
    if S >= 1024:
        assert ran >= 4 and chunked == 0, f"{what}: the equal-shares scan handed back ({ran} launches, {chunked} chunked)"
    else:
        assert ran == 0 and chunked >= 4, (ran, chunked)
    pb.judge(out, what)


# ---- the lean variants: heads, window, sinks, grouped K/V heads -------------------------------------------------------------------
# W 40 spans 64 tokens: one item per windowed row at chunk_tokens 64 (no body); W 100 spans 128: two items and the merge
LEAN = [("heads", 2, 2, 0, 0), ("window", 1, 1, 40, 0), ("window", 2, 2, 40, 0), ("window", 1, 1, 100, 0), ("window", 2, 2, 100, 0),
        ("sinks", 1, 1, 40, 4), ("sinks", 2, 2, 40, 4), ("gqa", 2, 1, 0, 0), ("gqa", 2, 1, 40, 4),
        # the biased and the capped scan (their own kernel families): plain, grouped under a window with sinks / a two-item window
        ("alibi", 2, 2, 0, 0), ("alibi", 2, 1, 40, 4), ("softcap", 2, 2, 0, 0), ("softcap", 2, 1, 100, 0)]
LEAN_FAMILY = {"alibi": "scan_heads_alibi", "softcap": "scan_heads_softcap"}


def _lean_grid():
    out = [(entry, elem, H, Hkv, W, K) for entry, H, Hkv, W, K in LEAN for elem in ("f32", "bf16")]
    return out + [("window", "fp8", 1, 1, 40, 0), ("window", "fp8", 1, 1, 100, 0)]


@pytest.mark.parametrize("entry,elem,H,Hkv,W,K", _lean_grid(), ids=lambda v: str(v))
def test_lean_variants(oracle, mli, dev, others, entry, elem, H, Hkv, W, K):
    B, S, D = 12, 256, 128
    L = length_vectors(1400 + H + W, B, S)[0]
    extra = {"alibi": dict(slopes=alm.standard_slopes(H)), "softcap": dict(cap=scm.CAPS[1])}.get(entry, {})
    pb = Paged(oracle, dev, 1500 + 7 * H + W + K, B, S, D, elem, "mixed" if H > 1 else "offset+", L, H, Hkv, W, K, **extra)
    need = heads_need(mli, pb)
    what = f"decode_scan_paged_{entry} {elem} ({B}, {S}, {D}) H {H} Hkv {Hkv} W {W} K {K}"
    other = others["plain" if H > 1 else "heads"]
    with knobs(mli, chunk_tokens=64):
        assert mli.mli_launch_counts_reset() == 0
        arena, out, _ = scan_case(mli, dev, pb, other, what, entry, need)
        assert launches(mli, LEAN_FAMILY.get(entry, "scan_heads_window")) >= 4, f"{what}: handed to another kernel"
        pb.judge(out, what)
        # the single-head call uses the same buffer directly afterwards, as "keep", then with a zero body: the same bits
        images = sf.save(arena, ["out"])
        plain = {}
        for fill in ("keep", "zero"):
            arena.fill("ws", fill, lo=COUNTERS)
            sf.restore(arena, images)
            rc = pb.scan(mli, arena, "", "plain", need)
            assert rc == 0, f"{what}: the single-head call afterwards returned {rc}"
            arena.assert_guards_intact(f"{what}, single head afterwards ({fill})")
            arena.assert_zero("ws", 0, COUNTERS, f"{what}, single head afterwards ({fill}): counters")
            plain[fill] = sf.bits(arena.view("out"))
        sf.assert_same_bits(plain["keep"], plain["zero"], f"{what}: single head on the multi-head call's leftovers")
    got = f32(plain["keep"], (B, D))
    check_rows(got, L, what + " single head")
    pb.judge(got, what + " single head", H=1, Hkv=1, W=0, K=0)


# ---- mli_decode_scan_contiguous and the softmax.V launchers ---------------------------------------------------------------------
class Contiguous:
    def __init__(self, oracle, seed, B, S, D, family, L):
        c = base_case(seed, B, S, D, L)
        self.B, self.S, self.D, self.L = B, S, D, c["lengths"]
        self.q, self.kt = apply_family(c, family)
        self.v = c["v_cache"].copy()
        poison_contiguous(self.q, self.kt, self.v, self.L)
        self.model = fm.Model(self.q, self.kt, self.v, self.L)
        self.o_oracle = oracle_scan(oracle, self.q, self.kt, self.v, self.L)[2]
        # softmax.V on its own: fed the model's probabilities rounded to fp32, so that the stage's error is its own
        self.p32 = self.model.p.astype(np.float32)
        self.pv = type("M", (), {})()
        self.pv.lengths, self.pv.o = self.model.lengths, fm.attend(self.p32, self.v, self.L)
        self.pv.o_scale = fm.attend_abs(self.p32, self.v, self.L).max(axis=1)
        self.pv_oracle = np.zeros((B, D), np.float32)
        oracle.softmax_v_host(self.p32, np.ascontiguousarray(self.v), self.pv_oracle, np.ascontiguousarray(self.L, np.int32))


def judge_attention(out, model, o_oracle, what):
    err, e_or = fm.attention_error(out, model), fm.attention_error(o_oracle, model)
    tol = fm.tolerance(e_or)
    print(f"SCRATCH {what} | attention: kernel {err.max():.3e}  oracle {e_or.max():.3e}  tol {tol:.3e}")
    assert err.max() <= tol, f"{what}: attention {err.max():.3e} > tol {tol:.3e} in rows {np.nonzero(~(err <= tol))[0][:8]}"


def run_simple(mli, dev, others, what, inputs, call, need, B, S, D, L, ladder_all_ok=False, knob=None):
    """A call with named inputs, one [B, D] output and the workspace; the other call is the multi-head scan."""
    other = others["heads"]
    n_other = heads_need(mli, other)
    arena = sf.Arena(sf.Arena.room(*[a.nbytes if isinstance(a, np.ndarray) else a.numel() * a.element_size()
                                    for a in inputs.values()], B * D * 4, *other.room(), max(need, n_other)), dev)
    for name, a in inputs.items():
        arena.carve_from(name, a)
    arena.carve("out", B * D * 4)
    arena.view("out", torch.float32).fill_(SENTINEL)
    carve_workspace(arena, other, need, n_other)
    with knobs(mli, **(knob or {})):
        first = contract(arena, what, lambda n: call(arena, n), sf.save(arena, ["out"]), ["out"], need,
                         other=other_call(mli, arena, other, need), ladder=True, ladder_all_ok=ladder_all_ok,
                         stats=stats_bytes(B, S))
    out = f32(first["out"], (B, D))
    check_rows(out, L, what)
    return arena, out


@pytest.mark.parametrize("S", [256, 512])
def test_decode_scan_contiguous(oracle, mli, dev, others, S):
    """One workgroup scores 256 tokens: n_sequence 256 is one item per row (no body: every size must do), 512 several."""
    B, D = 12, 64
    L = length_vectors(1600 + S, B, S)[0]
    c = Contiguous(oracle, 1601 + S, B, S, D, "late_peak", L)
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    what = f"decode_scan_contiguous ({B}, {S}, {D})"

    def call(arena, n):
        return mli.mli_decode_scan_contiguous(arena.ptr("q"), arena.ptr("kt"), arena.ptr("v"), arena.ptr("lengths"),
                                              arena.ptr("out"), B, S, D, arena.ptr("ws"), n, stream())
    _, out = run_simple(mli, dev, others, what, {"q": c.q, "kt": c.kt, "v": c.v, "lengths": c.L}, call, need, B, S, D, L,
                        ladder_all_ok=S == 256)
    judge_attention(out, c.model, c.o_oracle, what)


@pytest.mark.parametrize("D,chunk", [(64, 64), (64, 0), (66, 64)])
def test_softmax_v(oracle, mli, dev, others, D, chunk):
    """mli_softmax_v; emb_dim 66 is the scalar form."""
    B, S = 12, 256
    L = length_vectors(1700 + D, B, S)[0]
    c = Contiguous(oracle, 1701 + D, B, S, D, "flat", L)
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    what = f"softmax_v ({B}, {S}, {D}) chunk_tokens {chunk}"

    def call(arena, n):
        return mli.mli_softmax_v(arena.ptr("p"), arena.ptr("v"), arena.ptr("lengths"), arena.ptr("out"), B, S, D,
                                 arena.ptr("ws"), n, stream())
    _, out = run_simple(mli, dev, others, what, {"p": c.p32, "v": c.v, "lengths": c.L}, call, need, B, S, D, L,
                        knob={"chunk_tokens": chunk})
    judge_attention(out, c.pv, c.pv_oracle, what)


@pytest.mark.parametrize("elem", ["f32", "bf16"])
def test_softmax_v_paged(oracle, mli, dev, others, elem):
    """mli_softmax_v_paged and mli_softmax_v_paged_bf16."""
    B, S, D = 12, 256, 64
    L = length_vectors(1800, B, S)[0]
    pb = Paged(oracle, dev, 1801, B, S, D, elem, "flat", L)
    model = fm.Model(pb.q, pb.ktm, pb.v_rows, L)
    p32 = model.p.astype(np.float32)
    pv = type("M", (), {})()
    pv.lengths, pv.o, pv.o_scale = model.lengths, fm.attend(p32, pb.v_rows, L), fm.attend_abs(p32, pb.v_rows, L).max(axis=1)
    pv_oracle = np.zeros((B, D), np.float32)
    oracle.softmax_v_host(p32, np.ascontiguousarray(pb.v_rows, np.float32), pv_oracle, np.ascontiguousarray(L, np.int32))
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    what = f"softmax_v_paged {elem} ({B}, {S}, {D})"
    fn = mli.mli_softmax_v_paged if elem == "f32" else mli.mli_softmax_v_paged_bf16
    other = others["heads"]
    n_other = heads_need(mli, other)
    arena = sf.Arena(sf.Arena.room(p32.nbytes, *pb.room(), *other.room(), max(need, n_other)), dev)
    arena.carve_from("p", p32)
    pb.place(arena)
    carve_workspace(arena, other, need, n_other)

    def call(n):
        return fn(arena.ptr("p"), arena.ptr("table"), arena.ptr("lengths"), arena.ptr("out"), B, S, D, arena.ptr("ws"), n,
                  stream())
    with knobs(mli, chunk_tokens=64):
        first = contract(arena, what, call, sf.save(arena, ["out"]), ["out"], need, other=other_call(mli, arena, other, need),
                         ladder=True, stats=stats_bytes(B, S))
    out = f32(first["out"], (B, D))
    check_rows(out, L, what)
    judge_attention(out, pv, pv_oracle, what)


# ---- the compositions: fill (three new rows) -> latest -> scan ----------------------------------------------------------------------
def judge_memory(oracle, q, k_rows, v_rows, L, out, what, H=1, Hkv=1, W=0, K=0, slopes=None, cap=None):
    """e for a composition: attention_result against the float64 model of what the call left in memory -- its q_output and
    the K / V rows of the pages or caches, the appended row included -- tolerance from the fp32 oracle on the same (with
    slopes or a cap: alibi_model's / softcap_model's model and derived bound)."""
    ktm = np.ascontiguousarray(k_rows).transpose(0, 2, 1)
    if slopes is not None or cap is not None:
        m, arg = (alm, slopes) if slopes is not None else (scm, cap)
        model = (m.AlibiModel if m is alm else m.SoftcapModel)(q, ktm, v_rows, L, H, Hkv, arg, W, K)
        worst, tol = m.compare(out, m.eval_fp32(q, ktm, v_rows, L, H, Hkv, arg, W, K), model, what=what)
        assert worst <= tol, f"{what}: {worst:.3e} > tol {tol:.3e}"
        return
    model = gqa.model_gqa(q, ktm, v_rows, L, H, Hkv, W, K)
    o_or = gqa.oracle_gqa(oracle, np.ascontiguousarray(q), ktm, v_rows, L, H, Hkv, W, K)
    gqa.assert_within(gqa.compare(out, o_or, model, ("flat",) * H, what=what), what)


def page_values(raw, elem):
    """float32 values of the bytes of a page pool, as the kernels read them"""
    from helpers import fp8_decode
    if elem == "f32":
        return raw.view(np.float32)
    if elem == "bf16":
        return (raw.view(np.uint16).astype(np.uint32) << 16).view(np.float32)
    return fp8_decode(raw)


def place_all(arena, inputs, outputs):
    """inputs: name -> array (followed by a 0xFF guard); outputs: name -> (bytes, dtype, sentinel)"""
    for name, a in inputs.items():
        arena.carve_from(name, a)
    for name, (n, dtype, sentinel) in outputs.items():
        arena.carve(name, n)
        arena.view(name, dtype).fill_(sentinel)


def nbytes_of(a):
    return a.nbytes if isinstance(a, np.ndarray) else a.numel() * a.element_size()


def record_refusal(arena, what, call, need, images, scratch="ws"):
    """The fill-first compositions fill before they scan (and the decode steps attend before they decode): what they answer
    to need - 256 bytes of a scratch is recorded, not asserted; the guards hold whatever they answer."""
    n = max(need - 256, 0)
    arena.resize(scratch, n)
    sf.restore(arena, images)
    rc = call(n)
    arena.assert_guards_intact(f"{what}, {n} of {need} bytes")
    REFUSALS[what] = rc
    print(f"SCRATCH {what} | status with {n} of {need} bytes: {rc}")
    arena.resize(scratch, need)


def place_pool(arena, pool, table, elem, p="", tail="ff"):
    """The page pool between guards and the table of device pointers into it (table: element offsets, < 0 = no page)."""
    arena.carve_from(p + "pool", pool, tail=tail)
    arena.carve_from(p + "table", np.where(table >= 0, arena.address(p + "pool") + ESIZE[elem] * table, 0).astype(np.int64))


def carve_workspace(arena, other, need, n_other):
    """The other call's problem and, behind it, the workspace: the arena owns the larger of the two sizes from its start."""
    other.place(arena, "o.")
    arena.carve("ws", need, extent=max(need, n_other))


# (entry, page type, emb_dim, n_batch, fused_softmax).  At emb_dim 64 the materialising compositions run the single-pass scan
# (phases 3) and "fused_softmax" has nothing to decide.  The knob applies where that scan does not take the rows -- more than
# eight lane loads: fp32 beyond 2048, bf16 beyond 4096 columns -- and the composition goes through the separate passes:
# qkt with chunk statistics + softmax folded into softmax.V (1), or qkt, softmax, softmax.V (0).
PAGED_COMPOSITIONS = [("paged_attention", "f32", 64, 12, -1), ("paged_attention_bf16", "bf16", 64, 12, -1),
                      ("paged_attention", "f32", 2052, 8, 1), ("paged_attention", "f32", 2052, 8, 0),
                      ("paged_attention_bf16", "bf16", 4104, 8, 1), ("paged_attention_bf16", "bf16", 4104, 8, 0),
                      ("lean", "f32", 64, 12, -1), ("lean", "bf16", 64, 12, -1), ("lean", "fp8", 64, 12, -1),
                      ("lean_gqa", "f32", 128, 12, -1), ("lean_gqa", "bf16", 128, 12, -1),
                      # the biased, the capped and the rotated composition: two heads on one K/V head under W 40 with 4 sinks
                      ("lean_alibi", "f32", 128, 12, -1), ("lean_alibi", "bf16", 128, 12, -1),
                      ("lean_softcap", "f32", 128, 12, -1), ("lean_softcap", "bf16", 128, 12, -1),
                      ("lean_rope", "f32", 128, 12, -1), ("lean_rope", "bf16", 128, 12, -1)]
GROUPED = ("lean_gqa", "lean_alibi", "lean_softcap", "lean_rope")


@pytest.mark.parametrize("entry,elem,D,B,fused", PAGED_COMPOSITIONS, ids=lambda v: str(v))
def test_paged_compositions(oracle, mli, dev, others, entry, elem, D, B, fused):
    S, n_new = 256, 3
    H, Hkv, W, K = (2, 1, 40, 4) if entry in GROUPED else (1, 1, 0, 0)
    slopes = alm.standard_slopes(H) if entry == "lean_alibi" else None
    cap = scm.CAPS[1] if entry == "lean_softcap" else None
    L = length_vectors(1900 + D, B, S)[0]
    c = paged_case(1901 + D, B, S, D, conditioned=True, lengths=L)
    new_idx = c["new_batch_idx"].copy()
    new_idx[:n_new] = [1, 2, 4]                                    # rows of 1, 63 and 65 tokens are new: filled from x
    pool, _ = pages_on_device(oracle, dev, c, c["q_output"], c["kt_cache"], c["v_cache"], elem, "nan")
    w = {k: c[k] if elem == "f32" else bf16_bits(c[k]).reshape(D, D) for k in ("wk", "wq", "wv")}
    materialising = entry.startswith("paged_attention")
    need = int(mli.mli_attention_heads_workspace_bytes(B, S, D, H))
    other = others["heads" if H == 1 else "plain"]
    n_other = heads_need(mli, other)
    inputs = {"wk": w["wk"], "wq": w["wq"], "wv": w["wv"], "new_idx": new_idx, "lengths": L}
    if slopes is not None:
        inputs["slopes"] = slopes
    if entry == "lean_rope":
        import rope_model
        inputs["rope"] = rope_model.standard_table(S, D // H)
    outs = {"q": (B * D * 4, torch.float32, SENTINEL), "out": (B * D * 4, torch.float32, SENTINEL)}
    if materialising:
        outs["qkt"] = (B * S * 4, torch.float32, SENTINEL)
    arena = sf.Arena(sf.Arena.room(*[nbytes_of(a) for a in inputs.values()], *[n for n, _, _ in outs.values()],
                                   nbytes_of(pool), c["table"].size * 8, *other.room(), max(need, n_other)), dev)
    place_all(arena, inputs, outs)
    place_pool(arena, pool, c["table"], elem)
    carve_workspace(arena, other, need, n_other)
    a = arena.ptr
    front = (a("table"), a("lengths"), a("wk"), a("wq"), a("wv"), a("new_idx"), a("q"))

    def call(n):
        tail = (arena.ptr("ws"), n, stream())
        if entry == "paged_attention":
            return mli.mli_paged_attention(*front, a("qkt"), a("out"), B, S, D, n_new, *tail)
        if entry == "paged_attention_bf16":
            return mli.mli_paged_attention_bf16(*front, a("qkt"), a("out"), B, S, D, n_new, *tail)
        if entry == "lean":
            return mli.mli_paged_attention_lean(*front, a("out"), B, S, D, n_new, ELEM[elem], *tail)
        shape = (B, S, D, n_new, H, Hkv, W, K)
        if entry == "lean_alibi":
            return mli.mli_paged_attention_lean_alibi(*front, a("out"), *shape, a("slopes"), ELEM[elem], *tail)
        if entry == "lean_softcap":
            return mli.mli_paged_attention_lean_softcap(*front, a("out"), *shape, cap, None, ELEM[elem], *tail)
        if entry == "lean_rope":
            return mli.mli_paged_attention_lean_rope(*front, a("out"), *shape, None, a("rope"), ELEM[elem], *tail)
        return mli.mli_paged_attention_lean_gqa(*front, a("out"), B, S, D, n_new, H, Hkv, W, K, ELEM[elem], *tail)
    what = f"{entry} {elem} ({B}, {S}, {D})" + (f" H {H} Hkv {Hkv} W {W} K {K}" if H > 1 else "") + \
           (f" fused_softmax {fused}" if fused >= 0 else "")
    outputs = list(outs) + ["pool"]
    images = sf.save(arena, outputs)
    with knobs(mli, chunk_tokens=64, fused_softmax=fused):
        assert mli.mli_launch_counts_reset() == 0
        first = contract(arena, what, call, images, outputs, need, other=other_call(mli, arena, other, need))
        record_refusal(arena, what, call, need, images)
        family = {"lean_alibi": "scan_heads_alibi", "lean_softcap": "scan_heads_softcap", "lean_rope": "scan_heads_window"}.get(entry)
        if family:
            assert launches(mli, family) >= 3, f"{what}: handed to another kernel"
        if entry == "lean_rope":
            assert launches(mli, "gemm_f32_rope") + launches(mli, "gemm_bf16_rope") >= 6, f"{what}: fill and projection rotate"
        if materialising:     # which form ran: the single-pass scan counts as "scan_chunked", the separate passes as nothing
            assert (launches(mli, "scan_chunked") == 0) == (fused >= 0), f"{what}: {launches(mli, 'scan_chunked')} scan launches"
    out, q = f32(first["out"], (B, D)), f32(first["q"], (B, D))
    check_rows(out, L, what)
    assert np.isfinite(q).all() and not (q[L > 0] == SENTINEL).any(), f"{what}: q_output"
    values = page_values(first["pool"], elem)
    k_rows, v_rows = fm.gather_pages(values, c["table"], L, S, D, 1), fm.gather_pages(values, c["table"], L, S, D, 2)
    judge_memory(oracle, q, k_rows, v_rows, L, out, what, H, Hkv, W, K, slopes=slopes, cap=cap)
    if materialising:
        probs = f32(first["qkt"], (B, S))
        model = fm.Model(q, k_rows.transpose(0, 2, 1), v_rows, L)
        p_or = oracle_scan(oracle, np.ascontiguousarray(q), k_rows.transpose(0, 2, 1), v_rows, L)[1]
        err, e_or = fm.probability_error(probs, model), fm.probability_error(p_or, model)
        print(f"SCRATCH {what} | probabilities: kernel {err.max():.3e}  oracle {e_or.max():.3e}  tol {fm.tolerance(e_or):.3e}")
        assert err.max() <= fm.tolerance(e_or), f"{what}: probabilities"


@pytest.mark.parametrize("entry,S,fused", [("inference_self_attention", 256, 1), ("inference_self_attention", 256, 0),
                                           ("self_attention_lean", 256, -1), ("self_attention_lean", 512, -1)])
def test_contiguous_compositions(oracle, mli, dev, others, entry, S, fused):
    B, D, n_new = 12, 64, 3
    L = length_vectors(2000 + S, B, S)[0]
    c = paged_case(2001 + S, B, S, D, conditioned=True, lengths=L)
    new_idx = c["new_batch_idx"].copy()
    new_idx[:n_new] = [1, 2, 4]
    materialising = entry == "inference_self_attention"
    need = int(mli.mli_attention_workspace_bytes(B, S, D))
    other = others["heads"]
    n_other = heads_need(mli, other)
    inputs = {"inp": c["inp_embedding"], "wk": c["wk"], "wq": c["wq"], "wv": c["wv"], "new_idx": new_idx, "lengths": L}
    outs = {"q": (B * D * 4, torch.float32, SENTINEL), "out": (B * D * 4, torch.float32, SENTINEL)}
    if materialising:
        outs["qkt"] = (B * S * 4, torch.float32, SENTINEL)
    arena = sf.Arena(sf.Arena.room(*[nbytes_of(x) for x in inputs.values()], *[n for n, _, _ in outs.values()],
                                   c["kt_cache"].nbytes, c["v_cache"].nbytes, *other.room(), max(need, n_other)), dev)
    place_all(arena, inputs, outs)
    arena.carve_from("kt", c["kt_cache"], tail="pattern")
    arena.carve_from("v", c["v_cache"], tail="pattern")
    carve_workspace(arena, other, need, n_other)
    a = arena.ptr
    front = (a("inp"), a("lengths"), a("wk"), a("wq"), a("wv"), a("new_idx"), a("kt"), a("v"), a("q"))

    def call(n):
        tail = (B, S, D, D, n_new, arena.ptr("ws"), n, stream())
        if materialising:
            return mli.mli_inference_self_attention(*front, a("qkt"), a("out"), *tail)
        return mli.mli_self_attention_lean(*front, a("out"), *tail)
    what = f"{entry} ({B}, {S}, {D})" + (f" fused_softmax {fused}" if materialising else "")
    outputs = list(outs) + ["kt", "v"]
    images = sf.save(arena, outputs)
    with knobs(mli, fused_softmax=fused):
        first = contract(arena, what, call, images, outputs, need, other=other_call(mli, arena, other, need))
        record_refusal(arena, what, call, need, images)
    out, q = f32(first["out"], (B, D)), f32(first["q"], (B, D))
    check_rows(out, L, what)
    assert np.isfinite(q).all() and not (q[L > 0] == SENTINEL).any(), f"{what}: q_output"
    kt, v = f32(first["kt"], (B, D, S)), f32(first["v"], (B, S, D))
    model = fm.Model(q, kt, v, L)
    _, p_or, o_or = oracle_scan(oracle, np.ascontiguousarray(q), kt, v, L)
    judge_attention(out, model, o_or, what)
    if materialising:
        err, e_or = fm.probability_error(f32(first["qkt"], (B, S)), model), fm.probability_error(p_or, model)
        print(f"SCRATCH {what} | probabilities: kernel {err.max():.3e}  oracle {e_or.max():.3e}  tol {fm.tolerance(e_or):.3e}")
        assert err.max() <= fm.tolerance(e_or), f"{what}: probabilities"


# (layout, n_batch, n_sequence, emb_dim, fused_softmax).  mli_decode_step takes the materialising composition -- where
# "fused_softmax" applies -- for the rows its single-launch scan does not cover: more rows than half the arrival counters
# (8192) with several 256-token items per row.  8193 rows of 260 tokens and 4 columns is the smallest such shape.
DECODE_STEPS = [("contiguous", 12, 256, 64, -1), ("f32", 12, 256, 64, -1), ("bf16", 12, 256, 64, -1),
                ("contiguous", 8193, 260, 4, 1), ("contiguous", 8193, 260, 4, 0)]


@pytest.mark.parametrize("layout,B,S,D,fused", DECODE_STEPS, ids=lambda v: str(v))
def test_decode_steps(oracle, mli, dev, others, layout, B, S, D, fused):
    """mli_decode_step and mli_paged_decode_step: the workspace and the decoder scratch each under the three fills."""
    V = 200
    materialising = fused >= 0
    paged = layout != "contiguous"
    n_res, i_dec = (2, 1) if paged else (1, 0)
    L = length_vectors(2100, B, S)[0]
    c = paged_case(2101, B, S, D, conditioned=True, lengths=L)
    rng = np.random.default_rng(2102)
    emb = (rng.standard_normal((V, D)) * 0.1).astype(np.float32)
    wpe = rng.standard_normal((S, D)).astype(np.float32)
    need, need_d = int(mli.mli_attention_workspace_bytes(B, S, D)), int(mli.mli_decoder_scratch_bytes(B, V))
    other = others["heads"]
    n_other = heads_need(mli, other)
    w = {k: c[k] if layout != "bf16" else bf16_bits(c[k]).reshape(D, D) for k in ("wk", "wq", "wv")}
    inputs = {"wk": w["wk"], "wq": w["wq"], "wv": w["wv"], "emb": emb, "wpe": wpe}
    outs = {"q": (B * D * 4, torch.float32, SENTINEL), "out": (B * D * 4, torch.float32, SENTINEL),
            "res": (B * n_res * 4, torch.int32, ISENTINEL), "qkt": (B * S * 4, torch.float32, SENTINEL)}
    if paged:
        pool, _ = pages_on_device(oracle, dev, c, c["q_output"], c["kt_cache"], c["v_cache"], layout, "nan")
        state = [nbytes_of(pool), c["table"].size * 8]
    else:
        state = [c["inp_embedding"].nbytes, c["kt_cache"].nbytes, c["v_cache"].nbytes]
    arena = sf.Arena(sf.Arena.room(*[nbytes_of(x) for x in inputs.values()], *[n for n, _, _ in outs.values()], L.nbytes, *state,
                                   *other.room(), max(need, n_other), need_d), dev)
    place_all(arena, inputs, outs)
    arena.carve_from("lengths", L, tail="pattern")
    if paged:
        place_pool(arena, pool, c["table"], layout, tail="pattern")
        mutable = ["pool"]
    else:
        arena.carve_from("inp", c["inp_embedding"], tail="pattern")
        arena.carve_from("kt", c["kt_cache"], tail="pattern")
        arena.carve_from("v", c["v_cache"], tail="pattern")
        mutable = ["inp", "kt", "v"]
    carve_workspace(arena, other, need, n_other)
    arena.carve("dsc", need_d)
    a = arena.ptr

    def call(n, n_d=need_d):
        tail = (arena.ptr("ws"), n, arena.ptr("dsc"), n_d, stream())
        if paged:
            return mli.mli_paged_decode_step(a("table"), a("lengths"), a("wk"), a("wq"), a("wv"), a("emb"), a("wpe"), a("q"),
                                             a("out"), a("res"), B, S, D, V, n_res, i_dec, ELEM[layout], *tail)
        return mli.mli_decode_step(a("inp"), a("lengths"), a("wk"), a("wq"), a("wv"), a("emb"), a("wpe"), a("kt"), a("v"),
                                   a("q"), a("qkt"), a("out"), a("res"), B, S, D, V, *tail)
    what = f"{'paged_' if paged else ''}decode_step {layout} ({B}, {S}, {D}) V {V}" + (f" fused_softmax {fused}" if materialising else "")
    outputs = ["q", "out", "res", "lengths"] + mutable + (["qkt"] if materialising else [])
    images = sf.save(arena, outputs + ["qkt"])
    with knobs(mli, chunk_tokens=64, fused_softmax=fused):
        first = contract(arena, what + ": workspace", call, images, outputs, need, other=other_call(mli, arena, other, need))
        again = contract(arena, what + ": decoder scratch", lambda n_d: call(need, n_d), images, outputs, need_d, counters=0,
                         scratch="dsc")
        arena.assert_zero("ws", 0, COUNTERS, what)
        # attention first, then the head: with too little of either scratch the step may have run in part (recorded)
        record_refusal(arena, what + ": workspace", call, need, images)
        record_refusal(arena, what + ": decoder scratch", lambda n_d: call(need, n_d), need_d, images, scratch="dsc")
    for name in outputs:
        sf.assert_same_bits(again[name], first[name], f"{what}: {name} between the two protocols")
    # which composition ran: the single-launch scan leaves qkt_output alone, the materialising one leaves probabilities
    probs = f32(first["qkt"] if materialising else sf.bits(arena.view("qkt")), (B, S))
    if materialising:
        assert not (probs[np.arange(S)[None, :] < L[:, None]] == SENTINEL).any(), f"{what}: the lean composition ran"
    else:
        assert (probs == SENTINEL).all(), f"{what}: qkt_output was written"
    out, q = f32(first["out"], (B, D)), f32(first["q"], (B, D))
    check_rows(out, L, what)
    res = first["res"].view(np.int32).reshape(B, n_res)
    tok = res[:, i_dec]
    assert (tok[L == 0] == -1).all() and ((tok[L > 0] >= 0) & (tok[L > 0] < V)).all(), f"{what}: tokens {tok}"
    if paged:
        assert (res[:, 0] == ISENTINEL).all(), f"{what}: column 0 of decoder_result was written"
    new_len = first["lengths"].view(np.int32)
    want_len = np.where((L == 0) | (L + 1 >= S) | (tok == 1023), 0, L + 1)
    assert (new_len == want_len).all(), f"{what}: lengths {new_len} want {want_len}"
    if paged:
        values = page_values(first["pool"], layout)
        k_rows, v_rows = fm.gather_pages(values, c["table"], L, S, D, 1), fm.gather_pages(values, c["table"], L, S, D, 2)
        judge_memory(oracle, q, k_rows, v_rows, L, out, what)
        return
    kt, v = f32(first["kt"], (B, D, S)), f32(first["v"], (B, S, D))
    model = fm.Model(q, kt, v, L)
    _, p_or, o_or = oracle_scan(oracle, np.ascontiguousarray(q), kt, v, L)
    judge_attention(out, model, o_or, what)
    if materialising:
        err, e_or = fm.probability_error(probs, model), fm.probability_error(p_or, model)
        print(f"SCRATCH {what} | probabilities: kernel {err.max():.3e}  oracle {e_or.max():.3e}  tol {fm.tolerance(e_or):.3e}")
        assert err.max() <= fm.tolerance(e_or), f"{what}: probabilities"


# ---- decoder scratch ------------------------------------------------------------------------------------------------------------------
def decoder_pages(dev, c, layout):
    """Pages of a gemm_model.LogitsCase: a pool in the layout's element type and its table (element offsets)."""
    from min_llm_inference_amd import ops
    rng = np.random.default_rng(c.B + c.V)
    pool, table = build_page_pool(rng, c.L, c.S, c.D)
    if layout == "bf16":
        return torch.from_numpy(bf16_bits(pool).view(np.int16)).to(dev), table
    if layout == "fp8":
        return ops.f32_to_fp8(torch.from_numpy(pool).to(dev)), table
    return torch.from_numpy(pool).to(dev), table


def place_decoder(arena, dev, c, layout, n_res, p=""):
    arena.carve_from(p + "att", c.att)
    arena.carve_from(p + "emb", c.emb)
    arena.carve_from(p + "wpe", c.wpe)
    arena.carve_from(p + "lengths", c.L, tail="pattern")
    arena.carve(p + "res", c.B * n_res * 4)
    arena.view(p + "res", torch.int32).fill_(ISENTINEL)
    if layout == "contiguous":
        arena.carve_from(p + "inp", c.inp, tail="pattern")
        return [p + "res", p + "lengths", p + "inp"]
    pool, table = decoder_pages(dev, c, layout)
    place_pool(arena, pool, table, layout, p, tail="pattern")
    return [p + "res", p + "lengths", p + "pool"]


def decoder_room(c, n_res):
    return [c.att.nbytes, c.emb.nbytes, c.wpe.nbytes, c.L.nbytes, c.B * n_res * 4, c.inp.nbytes * 3 + 4096, c.B * (c.S // PAGE) * 8]


def fused_call(mli, arena, c, layout, n_res, i_dec, n, p="", scratch="dsc"):
    a = lambda name: arena.ptr(p + name)
    if layout == "contiguous":
        return mli.mli_decoder_fused(a("att"), a("emb"), a("wpe"), a("inp"), a("lengths"), a("res"), c.B, c.V, c.S, c.D,
                                     arena.ptr(scratch), n, stream())
    return mli.mli_paged_decoder_fused(a("att"), a("emb"), a("wpe"), a("table"), a("lengths"), a("res"), c.B, c.V, c.S, c.D,
                                       n_res, i_dec, ELEM[layout], arena.ptr(scratch), n, stream())


def other_decoder(mli, arena, dev, need):
    """The different call of the decoder cases -- another shape, the contiguous greedy head -- placed in the arena, the
    decoder scratch carved behind it; returns the call."""
    o = gm.LogitsCase(2300, "signed", 9, 77, 32)
    n_other = int(mli.mli_decoder_scratch_bytes(o.B, o.V))
    place_decoder(arena, dev, o, "contiguous", 1, "o.")
    arena.carve("dsc", need, extent=max(need, n_other))

    def run():
        arena.resize("dsc", n_other)
        rc = fused_call(mli, arena, o, "contiguous", 1, 0, n_other, "o.")
        arena.assert_guards_intact("the other call")
        arena.resize("dsc", need)
        return rc
    return run


OTHER_DECODER_ROOM = 9 * 32 * 32 * 4 * 4 + 77 * 32 * 4 + (1 << 16)     # what other_decoder carves, generously


def scores_of(mli, dev, c):
    """emb_score of the materialising head (the same GEMM), which judge_logits holds to the float64 product"""
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    score, res = t(c.score0), torch.zeros(c.B, dtype=torch.int32, device=dev)
    keep = (t(c.att), t(c.emb), t(c.wpe), t(c.inp), t(c.L))
    rc = mli.mli_decoder(ctypes.c_void_p(keep[0].data_ptr()), ctypes.c_void_p(keep[1].data_ptr()), ctypes.c_void_p(score.data_ptr()),
                         ctypes.c_void_p(keep[2].data_ptr()), ctypes.c_void_p(keep[3].data_ptr()), ctypes.c_void_p(keep[4].data_ptr()),
                         ctypes.c_void_p(res.data_ptr()), c.B, c.V, c.S, c.D, stream())
    assert rc == 0
    torch.cuda.synchronize()
    return score.cpu().numpy(), res.cpu().numpy()


DECODER_SHAPES = [(70, 1030, 64, {}, "panel"), (70, 1030, 64, {"gemm_panel": 0}, "tiles64"),
                  (130, 1030, 64, {"gemm_tall_tiles": 2}, "tall")]


@pytest.mark.parametrize("layout", ["contiguous", "f32", "bf16", "fp8"])
@pytest.mark.parametrize("B,V,D,knob,name", DECODER_SHAPES, ids=lambda v: v if isinstance(v, str) else None)
def test_decoder_fused(oracle, mli, dev, layout, B, V, D, knob, name):
    """mli_decoder_fused and mli_paged_decoder_fused: 32-column panel tiles, 64-column tiles and 128-row tiles over the
    (max, index) pairs of mli_decoder_scratch_bytes."""
    n_res, i_dec = (1, 0) if layout == "contiguous" else (2, 1)
    c = gm.LogitsCase(2200 + B, "signed", B, V, D)
    need = int(mli.mli_decoder_scratch_bytes(B, V))
    assert need > 0
    arena = sf.Arena(sf.Arena.room(*decoder_room(c, n_res), OTHER_DECODER_ROOM, need), dev)
    outputs = place_decoder(arena, dev, c, layout, n_res)
    other = other_decoder(mli, arena, dev, need)
    what = f"decoder_fused {layout} ({B}, V {V}, {D}) {name}"
    with knobs(mli, **knob):
        first = contract(arena, what, lambda n: fused_call(mli, arena, c, layout, n_res, i_dec, n), sf.save(arena, outputs),
                         outputs, need, other=other, counters=0, scratch="dsc", ladder=True)
        score, tok_unfused = scores_of(mli, dev, c)
    res = first["res"].view(np.int32).reshape(B, n_res)
    if n_res == 2:
        arena.assert_column_is("res", torch.int32, B, 2, 0, ISENTINEL, what)       # (the last call's, in the arena)
    fig = gm.Figures(what)
    gm.judge_logits(fig, oracle, c, score, res[:, i_dec], tok_unfused)
    fig.done()
    tok = res[:, i_dec]
    want_len = np.where((c.L == 0) | (c.L + 1 >= c.S) | (tok == 1023), 0, c.L + 1)
    assert (first["lengths"].view(np.int32) == want_len).all(), f"{what}: lengths"


@pytest.mark.parametrize("n_top", [None, 0, 8], ids=lambda v: "plain" if v is None else f"logprobs{v}")
@pytest.mark.parametrize("layout", ["contiguous", "f32", "bf16", "fp8"])
def test_decoder_sampled(oracle, mli, dev, layout, n_top):
    """mli_decoder_sampled, mli_paged_decoder_sampled and their _logprobs forms: the logits in the front of the scratch."""
    B, V, D = 24, 1030, 64
    plain_contiguous = layout == "contiguous" and n_top is None       # the one form without n_decoder_results
    n_res, i_dec = (1, 0) if plain_contiguous else (2, 1)
    c = gm.LogitsCase(2400, "signed", B, V, D)
    rng = np.random.default_rng(2401)
    T = rng.choice(np.array([0.0, 0.7, 1.1], np.float32), B)
    K = rng.choice(np.array([0, 40], np.int32), B)
    P = rng.choice(np.array([1.0, 0.9], np.float32), B)
    seed = rng.integers(0, 2 ** 62, B).astype(np.int64)
    need = int(mli.mli_decoder_sampled_scratch_bytes(B, V))
    top = max(n_top or 0, 1)
    arena = sf.Arena(sf.Arena.room(*decoder_room(c, n_res), OTHER_DECODER_ROOM, T.nbytes, K.nbytes, P.nbytes, seed.nbytes,
                                   B * n_res * 4, B * n_res * top * 4, B * n_res * top * 4, B * 4, need), dev)
    outputs = place_decoder(arena, dev, c, layout, n_res)
    for name, x in (("T", T), ("K", K), ("P", P), ("seed", seed)):
        arena.carve_from(name, x)
    if n_top is not None:
        place_all(arena, {}, {"lp": (B * n_res * 4, torch.float32, SENTINEL), "ids": (B * n_res * top * 4, torch.int32, ISENTINEL),
                              "tops": (B * n_res * top * 4, torch.float32, SENTINEL)})
        outputs += ["lp", "ids", "tops"]
    arena.carve("tok2", B * 4)
    other = other_decoder(mli, arena, dev, need)
    a = arena.ptr
    what = f"decoder_sampled {layout} ({B}, V {V}, {D}) " + ("plain" if n_top is None else f"logprobs n_top {n_top}")

    def call(n):
        params, tail = (a("T"), a("K"), a("P"), a("seed")), (arena.ptr("dsc"), n, stream())
        lp = () if n_top is None else (a("lp"), a("ids") if n_top else None, a("tops") if n_top else None, n_top)
        if layout == "contiguous":
            head = (a("att"), a("emb"), a("wpe"), a("inp"), a("lengths"), a("res"), B, V, c.S, D)
            if n_top is None:
                return mli.mli_decoder_sampled(*head, *params, *tail)
            return mli.mli_decoder_sampled_logprobs(*head, n_res, i_dec, *params, *lp, *tail)
        head = (a("att"), a("emb"), a("wpe"), a("table"), a("lengths"), a("res"), B, V, c.S, D, n_res, i_dec, ELEM[layout])
        if n_top is None:
            return mli.mli_paged_decoder_sampled(*head, *params, *tail)
        return mli.mli_paged_decoder_sampled_logprobs(*head, *params, *lp, *tail)

    first = contract(arena, what, call, sf.save(arena, outputs), outputs, need, other=other, counters=0, scratch="dsc", ladder=True)
    # the logits the head computed are the front of its scratch; the draw on them is mli_sample_tokens's, bit for bit
    logits = f32(sf.bits(arena.view("dsc"))[:B * V * 4], (B, V)).copy()
    res = first["res"].view(np.int32).reshape(B, n_res)
    tok = res[:, i_dec]
    sf.restore(arena, {"lengths": torch.from_numpy(c.L).to(dev).view(torch.uint8)})
    rc = mli.mli_sample_tokens(arena.ptr("dsc"), a("T"), a("K"), a("P"), a("seed"), a("lengths"), a("tok2"), B, V, None, 0, stream())
    assert rc == 0
    arena.assert_guards_intact(what + ", sample_tokens")
    assert (sf.bits(arena.view("tok2")).view(np.int32) == tok).all(), f"{what}: tokens differ from mli_sample_tokens on the same logits"
    sampling_cases.check_against_reference(logits, T, K, P, seed, c.L, tok, what)
    fig = gm.Figures(what)
    want, scale = gm.logits(c.att, c.emb)
    fig.check("logits in the scratch", gm.fp32_error(logits, want, scale),
              gm.fp32_error(gm.oracle_product(oracle, c.att, c.emb.T), want, scale), c.D)
    fig.done()
    if n_res == 2:
        arena.assert_column_is("res", torch.int32, B, 2, 0, ISENTINEL, what)
    if n_top is not None:
        arena.assert_column_is("lp", torch.float32, B, 2, 0, SENTINEL, what)
        if n_top:
            arena.assert_column_is("ids", torch.int32, B, 2, 0, ISENTINEL, what)
            arena.assert_column_is("tops", torch.float32, B, 2, 0, SENTINEL, what)
        lp = f32(first["lp"], (B, 2))[:, 1]
        ids = np.zeros((B, 0), np.int32)
        tops = np.zeros((B, 0), np.float32)
        if n_top:
            ids = first["ids"].view(np.int32).reshape(B, 2, n_top)
            tops = f32(first["tops"], (B, 2, n_top))
            ids, tops = ids[:, 1], tops[:, 1]
        err, tol, complaints = lpm.compare((lp, ids, tops), logits, tok, n_top)
        print(f"SCRATCH {what} | logprobs: error {err:.3e}  tol {tol:.3e}")
        assert not complaints and err <= tol, (what, err, tol, complaints)


# ---- entry points without scratch: the outputs are still fenced ------------------------------------------------------------------------
def test_qkt_and_softmax_in_place(oracle, mli, dev):
    """mli_qkt (writes nothing at s >= L) and mli_softmax_in_place_with_lengths (writes the whole row)."""
    B, S, D = 12, 256, 64
    L = length_vectors(2500, B, S)[0]
    c = Contiguous(oracle, 2501, B, S, D, "peaked", L)
    x_or = oracle_scan(oracle, c.q, c.kt, c.v, L)[0]
    arena = sf.Arena(sf.Arena.room(c.q.nbytes, c.kt.nbytes, L.nbytes, B * S * 4), dev)
    place_all(arena, {"q": c.q, "kt": c.kt, "lengths": L}, {"qkt": (B * S * 4, torch.float32, SENTINEL)})
    a = arena.ptr
    assert mli.mli_qkt(a("q"), a("kt"), a("lengths"), a("qkt"), B, S, D, stream()) == 0
    arena.assert_guards_intact("mli_qkt")
    x = f32(sf.bits(arena.view("qkt")), (B, S))
    dead = np.arange(S)[None, :] >= L[:, None]
    assert (x[dead] == SENTINEL).all() and np.isfinite(x[~dead]).all() and not (x[~dead] == SENTINEL).any()
    err, e_or = fm.score_error(x, c.model), fm.score_error(x_or, c.model)
    assert err.max() <= fm.tolerance(e_or), ("mli_qkt", err.max(), fm.tolerance(e_or))
    # the softmax in place, on the model's scores rounded to fp32 with dead scores that would dominate if they were read
    x32 = c.model.x.astype(np.float32)
    x32[dead] = 80.0
    ms = type("M", (), {})()
    ms.lengths, ms.p = c.model.lengths, fm.softmax(x32.astype(np.float64), L)
    p_or = x32.copy()
    oracle.softmax_in_place_with_lengths_host(p_or, np.ascontiguousarray(L, np.int32))
    arena.put("qkt", x32)
    assert mli.mli_softmax_in_place_with_lengths(a("qkt"), a("lengths"), B, S, stream()) == 0
    arena.assert_guards_intact("mli_softmax_in_place_with_lengths")
    err, e_or = fm.probability_error(f32(sf.bits(arena.view("qkt")), (B, S)), ms), fm.probability_error(p_or, ms)
    assert err.max() <= fm.tolerance(e_or), ("mli_softmax_in_place_with_lengths", err.max(), fm.tolerance(e_or))


def test_qkt_paged_and_latest(oracle, mli, dev):
    """mli_qkt_paged and mli_get_latest_k_q_v_paged: q_output, scores and the pool between guards."""
    B, S, D = 12, 256, 64
    L = length_vectors(2600, B, S)[0]
    pb = Paged(oracle, dev, 2601, B, S, D, "f32", "offset+", L)
    model = fm.Model(pb.q, pb.ktm, pb.v_rows, L)
    x_or = oracle_scan(oracle, pb.q, pb.ktm, pb.v_rows, L)[0]
    arena = sf.Arena(sf.Arena.room(*pb.room(True)), dev)
    pb.place(arena, "", True)
    a = arena.ptr
    assert mli.mli_qkt_paged(a("q"), a("table"), a("lengths"), a("qkt"), B, S, D, stream()) == 0
    arena.assert_guards_intact("mli_qkt_paged")
    x = f32(sf.bits(arena.view("qkt")), (B, S))
    dead = np.arange(S)[None, :] >= L[:, None]
    assert (x[dead] == SENTINEL).all() and np.isfinite(x[~dead]).all() and not (x[~dead] == SENTINEL).any()
    err, e_or = fm.score_error(x, model), fm.score_error(x_or, model)
    assert err.max() <= fm.tolerance(e_or), ("mli_qkt_paged", err.max(), fm.tolerance(e_or))
    # the decode projection: q to q_output, k and v appended to the page; nothing else of the pool changes
    c = paged_case(2602, B, S, D, conditioned=True, lengths=L)
    pool, _ = pages_on_device(oracle, dev, c, c["q_output"], c["kt_cache"], c["v_cache"], "f32", "nan")
    arena = sf.Arena(sf.Arena.room(nbytes_of(pool), c["table"].size * 8, L.nbytes, c["wk"].nbytes, c["wq"].nbytes, c["wv"].nbytes,
                                   B * D * 4), dev)
    place_all(arena, {"wk": c["wk"], "wq": c["wq"], "wv": c["wv"], "lengths": L}, {"q": (B * D * 4, torch.float32, SENTINEL)})
    arena.carve_from("pool", pool, tail="pattern")
    arena.carve_from("table", np.where(c["table"] >= 0, arena.address("pool") + 4 * c["table"], 0).astype(np.int64))
    before = sf.bits(arena.view("pool")).view(np.uint32).copy()
    a = arena.ptr
    assert mli.mli_get_latest_k_q_v_paged(a("table"), a("lengths"), a("wk"), a("wq"), a("wv"), a("q"), B, S, D, stream()) == 0
    arena.assert_guards_intact("mli_get_latest_k_q_v_paged")
    q = f32(sf.bits(arena.view("q")), (B, D))
    after = sf.bits(arena.view("pool")).view(np.uint32)
    q64, k64, v64, q_scale, k_scale, v_scale = fm.project_latest(c["inp_embedding"], L, c["wk"], c["wq"], c["wv"])
    o = {k: c[k].copy() for k in ("kt_cache", "v_cache", "q_output")}
    oracle.get_latest_kt_q_v(c["inp_embedding"], L, c["wk"], c["wq"], c["wv"], o["kt_cache"], o["v_cache"], o["q_output"])
    assert (q[L == 0] == SENTINEL).all() and np.isfinite(q[L > 0]).all()
    err, e_or = fm.projection_error(q, q64, L, q_scale), fm.projection_error(o["q_output"], q64, L, q_scale)
    assert err.max() <= fm.tolerance(e_or), ("q_output", err.max(), fm.tolerance(e_or))
    allowed = np.zeros(before.shape, bool)
    for b in np.nonzero(L > 0)[0]:
        s = int(L[b]) - 1
        off = int(c["table"][b, s // PAGE]) + (s % PAGE) * 3 * D + D
        allowed[off:off + 2 * D] = True
        got = after[off:off + 2 * D].view(np.float32).astype(np.float64)
        ek = np.abs(got[:D] - k64[b]).max() / k_scale[b]
        ev = np.abs(got[D:] - v64[b]).max() / v_scale[b]
        ok = np.abs(o["kt_cache"][b, :, s] - k64[b]).max() / k_scale[b]
        ov = np.abs(o["v_cache"][b, s] - v64[b]).max() / v_scale[b]
        assert ek <= fm.tolerance(ok) and ev <= fm.tolerance(ov), (b, ek, ev)
    assert (after[~allowed] == before[~allowed]).all(), "the projection changed the pool outside the appended K / V rows"


@pytest.mark.parametrize("elem", ["f32", "bf16", "fp8"])
def test_paged_prefill(oracle, mli, dev, elem):
    """mli_paged_prefill of three new rows: the pool between guards; only the live slots of the new rows change, and they hold
    x = emb[token] + wpe[s], x . Wk and x . Wv in the page element type."""
    B, S, D, V, n_new = 12, 256, 64, 300, 3
    L = length_vectors(2700, B, S)[0]
    rng = np.random.default_rng(2701)
    new_idx = np.zeros(B, np.int32)
    new_idx[:n_new] = [2, 4, 6]                                   # 63, 65 and S tokens
    emb = (rng.random((V, D), dtype=np.float32) * 2 - 1).astype(np.float32)
    wpe = (rng.random((S, D), dtype=np.float32) * 2 - 1).astype(np.float32)
    inp = rng.integers(0, V, size=(B, S)).astype(np.int32)
    w32 = [((rng.random((D, D), dtype=np.float32) * 2 - 1) / np.sqrt(D)).astype(np.float32) for _ in range(2)]
    w = w32 if elem == "f32" else [bf16_bits(x).reshape(D, D) for x in w32]
    page_bytes = PAGE * 3 * D * ESIZE[elem]
    pool = rng.integers(0, 256, size=B * (S // PAGE) * page_bytes, dtype=np.uint8)     # random bytes, NaN patterns included
    table = np.arange(B * (S // PAGE), dtype=np.int64).reshape(B, S // PAGE) * page_bytes
    arena = sf.Arena(sf.Arena.room(emb.nbytes, wpe.nbytes, inp.nbytes, w[0].nbytes, w[1].nbytes, L.nbytes, new_idx.nbytes, pool.nbytes,
                                   table.nbytes), dev)
    place_all(arena, {"emb": emb, "wpe": wpe, "inp": inp, "wk": w[0], "wv": w[1], "lengths": L, "new_idx": new_idx}, {})
    arena.carve_from("pool", pool, tail="pattern")
    arena.carve_from("table", arena.address("pool") + table)
    a = arena.ptr
    rc = mli.mli_paged_prefill(a("emb"), a("wpe"), a("inp"), a("table"), a("lengths"), a("new_idx"), a("wk"), a("wv"), B, S, D,
                               n_new, ELEM[elem], stream())
    assert rc == 0
    arena.assert_guards_intact(f"mli_paged_prefill {elem}")
    after = sf.bits(arena.view("pool"))
    live = np.zeros(pool.shape, bool)
    row_bytes = 3 * D * ESIZE[elem]
    w64 = [gm.decode(x, "f32" if elem == "f32" else "bf16").astype(np.float64) for x in w]
    for b in new_idx[:n_new]:
        n = min(int(L[b]), S)
        offs = [int(table[b, s // PAGE]) + (s % PAGE) * row_bytes for s in range(n)]
        for off in offs:
            live[off:off + row_bytes] = True
        stored = np.stack([after[off:off + row_bytes] for off in offs]).view(gm.BITS[elem]).reshape(n, 3, D)
        # x = emb[token] + wpe[s], one fp32 addition, stored in the page element type: exact.  K and V are products of the x
        # the kernel reads back from that type (gemm_model.Case.x_rows)
        x32 = (emb[inp[b, :n]] + wpe[:n]).astype(np.float32)
        assert (stored[:, 0] == gm.raw_bits(gm.encode(x32, elem), elem)).all(), f"prefill {elem}: x segment of row {b}"
        x_read = gm.round_to(x32, elem)
        fig = gm.Figures(f"paged_prefill {elem} row {b}")
        for seg in (1, 2):
            want, scale = gm.product(x_read, w64[seg - 1])
            e_or = gm.fp32_error(gm.oracle_product(oracle, x_read, w64[seg - 1]), want, scale)
            got = gm.decode(stored[:, seg].view(np.float32) if elem == "f32" else stored[:, seg], elem)
            fig.check(f"segment {seg}", gm.stored_error(got, want, scale, elem), e_or, D)
        fig.done()
    assert (after[~live] == pool[~live]).all(), f"prefill {elem}: bytes outside the live slots of the new rows changed"


@pytest.mark.parametrize("V", [1030, 15360])
def test_sample_tokens(mli, dev, V):
    """mli_sample_tokens needs no scratch; V 15360 is the largest row that is staged in LDS.  The logits are followed by a
    0xFF guard: a read past a row's end would put a NaN among the candidates of the last row."""
    B = 64
    x, T, K, P, seed, lengths = sampling_cases.drawn_case(np.random.default_rng(2800 + V), B, V)
    assert int(mli.mli_sample_scratch_bytes(B, V)) == 0
    arena = sf.Arena(sf.Arena.room(x.nbytes, T.nbytes, K.nbytes, P.nbytes, seed.nbytes, lengths.nbytes, B * 4), dev)
    place_all(arena, {"x": x, "T": T, "K": K, "P": P, "seed": seed.astype(np.int64), "lengths": lengths},
              {"tok": (B * 4, torch.int32, ISENTINEL)})
    a = arena.ptr
    runs = []
    for _ in range(2):
        arena.view("tok", torch.int32).fill_(ISENTINEL)
        rc = mli.mli_sample_tokens(a("x"), a("T"), a("K"), a("P"), a("seed"), a("lengths"), a("tok"), B, V, None, 0, stream())
        assert rc == 0
        arena.assert_guards_intact(f"mli_sample_tokens V {V}")
        runs.append(sf.bits(arena.view("tok")).view(np.int32))
    assert (runs[0] == runs[1]).all()
    sampling_cases.check_against_reference(x, T, K, P, seed, lengths, runs[0], f"sample_tokens V={V}")
    assert (runs[0][lengths == 0] == -1).all() and not (runs[0] == ISENTINEL).any()


# ---- mli_paged_prompt_logprobs[_softcap]: five regions carved from one scratch buffer -----------------------------------------------
PROMPT_CALLS = [(elem, H, Hkv, n_top, capped) for elem in ("f32", "bf16") for H, Hkv in ((1, 1), (4, 2)) for n_top in (0, 8)
                for capped in (False, True) if H > 1 or not capped]
WORKSPACE = -12          # MLI_ERR_WORKSPACE


def _segment_arrays(segs):
    """(rows, first, count, offset) int32 of [(row, first, count)] with dense offsets in list order, and the positions in all"""
    counts = [n for _, _, n in segs]
    off = np.concatenate([[0], np.cumsum(counts)[:-1]])
    return [np.asarray(a, np.int32) for a in ([r for r, _, _ in segs], [f for _, f, _ in segs], counts, off)], int(sum(counts))


@pytest.mark.parametrize("elem,H,Hkv,n_top,capped", PROMPT_CALLS, ids=lambda v: str(v))
def test_paged_prompt_logprobs(oracle, mli, dev, elem, H, Hkv, n_top, capped):
    """(4, 64, 128) with n_vocab 1030: pages, tokens, Wq, the embedding table, the segment arrays, the three output arrays and
    the scratch (gathered x | q | attention | logits | targets) in one arena.  Exactly mli_prompt_logprobs_scratch_bytes is
    enough; with 256 bytes fewer the call answers MLI_ERR_WORKSPACE and not one byte of the arena has changed; the guards are
    intact; the outputs are bit-identical with the scratch body zero, 0xFF and left behind by a call of another shape; the
    figures are within prompt_model.compare_given of the float64 forward over what the pages hold; the output rows of a
    segment the device checks skip (its row lies outside the batch) keep their sentinels.  "scan_prompt" /
    "scan_prompt_softcap" counts the scan."""
    B, S, D, V = 4, 64, 128, 1030
    cap = scm.CAPS[1] if capped else None
    L = np.asarray([63, 40, 17, 33], np.int32)
    c = paged_case(2800 + H, B, S, D, conditioned=True, lengths=L)
    pool, values = pages_on_device(oracle, dev, c, c["q_output"], c["kt_cache"], c["v_cache"], elem, "nan")
    rng = np.random.default_rng(2801 + H)
    emb = (rng.standard_normal((V, D)) * 0.5).astype(np.float32)
    inp = rng.integers(0, V, size=(B, S)).astype(np.int32)
    w32 = (rng.standard_normal((D, D)) * (2.0 / np.sqrt(D))).astype(np.float32)
    wq = w32 if elem == "f32" else bf16_bits(w32).reshape(D, D)
    w_values = gm.decode(wq, "f32" if elem == "f32" else "bf16").astype(np.float64)
    # the third segment names row 7 of a batch of 4: skipped whole by every kernel of the call
    segs = [(2, 0, 17), (0, 50, 13), (7, 0, 4), (3, 5, 20), (0, 20, 9)]
    arrays, n = _segment_arrays(segs)
    skipped = np.zeros(n, bool)
    skipped[int(arrays[3][2]):int(arrays[3][2]) + 4] = True
    other_segs = [(1, 3, 30), (3, 0, 2)]
    o_arrays, o_n = _segment_arrays(other_segs)
    V_other = 515
    need = int(mli.mli_prompt_logprobs_scratch_bytes(n, D, V))
    n_other = int(mli.mli_prompt_logprobs_scratch_bytes(o_n, D, V_other))
    assert 0 < n_other < need
    inputs = {"inp": inp, "wq": wq, "emb": emb}
    inputs.update({f"seg{i}": a for i, a in enumerate(arrays)})
    inputs.update({f"o.seg{i}": a for i, a in enumerate(o_arrays)})
    outs = {"lp": (n * 4, torch.float32, SENTINEL), "o.lp": (o_n * 4, torch.float32, SENTINEL)}
    if n_top:
        outs.update({"ids": (n * n_top * 4, torch.int32, ISENTINEL), "tops": (n * n_top * 4, torch.float32, SENTINEL)})
    arena = sf.Arena(sf.Arena.room(*[nbytes_of(a) for a in inputs.values()], *[b for b, _, _ in outs.values()], nbytes_of(pool),
                                   c["table"].size * 8, need), dev)
    place_all(arena, inputs, outs)
    place_pool(arena, pool, c["table"], elem)
    arena.carve("ws", need)
    a = arena.ptr

    def run(p, lp, n_pos, vocab, top, count, n_seg, scratch_bytes):
        front = (a("table"), a("inp"), a("wq"), a("emb"), a(p + "seg0"), a(p + "seg1"), a(p + "seg2"), a(p + "seg3"), a(lp),
                 a("ids") if top else None, a("tops") if top else None)
        shape = (n_seg, count, n_pos, B, S, D, vocab, H, Hkv, 0, 0)
        tail = (ELEM[elem], top, arena.ptr("ws"), scratch_bytes, stream())
        if capped:
            return mli.mli_paged_prompt_logprobs_softcap(*front, *shape, cap, *tail)
        return mli.mli_paged_prompt_logprobs(*front, *shape, *tail)

    def call(nbytes):
        return run("", "lp", n, V, n_top, 20, len(segs), nbytes)

    def other():
        arena.resize("ws", n_other)
        rc = run("o.", "o.lp", o_n, V_other, 0, 30, len(other_segs), n_other)
        arena.assert_guards_intact("the other call")
        arena.resize("ws", need)
        return rc

    what = f"paged_prompt_logprobs{'_softcap' if capped else ''} {elem} ({B}, {S}, {D}, {V}) H {H} Hkv {Hkv} n_top {n_top}"
    outputs = [k for k in outs if not k.startswith("o.")]
    images = sf.save(arena, outputs)
    assert mli.mli_launch_counts_reset() == 0
    first = contract(arena, what, call, images, outputs, need, other=other, counters=0)
    family, idle = ("scan_prompt_softcap", "scan_prompt") if capped else ("scan_prompt", "scan_prompt_softcap")
    assert launches(mli, family) == 4 and launches(mli, idle) == 0, f"{what}: three calls and the other one, handed to another kernel"
    rungs = sf.run_ladder(arena, "ws", [need - 256, need], call, images, outputs, first, 0, what)
    assert rungs == [(need - 256, WORKSPACE), (need, 0)], rungs
    # the skipped segment's rows keep their sentinels in every output array
    lp = f32(first["lp"], (n,))
    assert (lp[skipped] == SENTINEL).all(), f"{what}: token_logprob of a skipped segment was written: {lp[skipped]}"
    ids = tops = np.zeros((n, 0))
    if n_top:
        ids, tops = first["ids"].view(np.int32).reshape(n, n_top), f32(first["tops"], (n, n_top))
        assert (ids[skipped] == ISENTINEL).all() and (tops[skipped] == SENTINEL).all(), f"{what}: top_* of a skipped segment"
    # the float64 forward over what the pages hold: q = x . Wq, the causal scan, attention . emb^T
    live = [s for s in segs if s[0] < B]
    rows, pos = pm.queries(live)
    x_rows = fm.gather_pages(values, c["table"], L, S, D, 0).astype(np.float64)
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    q64 = x_rows[rows, pos] @ w_values
    if capped:
        attn = scm.prompt_model(q64, ktm, v_rows, rows, pos, H, Hkv, cap).o
    else:
        attn = pm.scan_float64(q64, ktm, v_rows, rows, pos, H, Hkv, 0, 0)
    logits = (attn @ emb.astype(np.float64).T).astype(np.float32)
    given = np.asarray([inp[r, t + 1] if t + 1 < S else -1 for r, t in zip(rows, pos)], np.int64)
    err, tol, bad = pm.compare_given((lp[~skipped], ids[~skipped], tops[~skipped]), logits, given, n_top)
    print(f"SCRATCH {what} | figures: error {err:.3e}  tolerance {tol:.3e}")
    assert not bad and err <= tol, (what, err, tol, bad)


# ---- entry points without scratch: the prompt projection and the prompt scan ---------------------------------------------------------
@pytest.mark.parametrize("elem,H,Hkv", [("f32", 1, 1), ("bf16", 1, 1), ("f32", 4, 2), ("bf16", 4, 2)])
def test_prompt_project_q_and_scan(oracle, mli, dev, elem, H, Hkv):
    """mli_prompt_project_q, then mli_prompt_scan_paged on its q, at (4, 64, 128) under W 40 with 4 sinks: pages, Wq, the segment
    arrays, `gathered`, q and the scan's output between guards (b); a dense row that belongs to no query keeps its sentinel
    in the scan's output, every row of a query is finite (d); q against float64 x . Wq at the fp32 chain's own bound
    D 2^-24 sum |x w|, the attention against the float64 model of what the pages hold and the q the projection left (e).
    "gemm_f32_rows64" / "gemm_bf16_widened" and "scan_prompt" count the launches."""
    B, S, D, W, K = 4, 64, 128, 40, 4
    L = np.asarray([63, 40, 17, 33], np.int32)
    c = paged_case(2900 + H, B, S, D, conditioned=True, lengths=L)
    pool, values = pages_on_device(oracle, dev, c, c["q_output"], c["kt_cache"], c["v_cache"], elem, "nan")
    w32 = ((np.random.default_rng(2901).random((D, D), dtype=np.float32) * 2 - 1) / np.sqrt(D)).astype(np.float32)
    wq = w32 if elem == "f32" else bf16_bits(w32).reshape(D, D)
    segs = [(2, 0, 17), (0, 50, 13), (3, 5, 20), (0, 20, 9)]
    arrays, n = _segment_arrays(segs)
    arrays[3][2:] += 1                                    # a hole of one dense row behind the second segment
    n_q = n + 2                                           # ... and a tail
    rows, pos = pm.queries(segs)
    where = np.concatenate([np.arange(o, o + cnt) for o, cnt in zip(arrays[3], arrays[2])])
    nobody = np.setdiff1d(np.arange(n_q), where)
    inputs = {"wq": wq}
    inputs.update({f"seg{i}": a for i, a in enumerate(arrays)})
    outs = {"gathered": (n_q * D * ESIZE[elem], torch.uint8, 0xFF), "q": (n_q * D * 4, torch.float32, SENTINEL),
            "out": (n_q * D * 4, torch.float32, SENTINEL)}
    arena = sf.Arena(sf.Arena.room(*[nbytes_of(a) for a in inputs.values()], *[b for b, _, _ in outs.values()], nbytes_of(pool),
                                   c["table"].size * 8), dev)
    place_all(arena, inputs, outs)
    place_pool(arena, pool, c["table"], elem)
    a = arena.ptr
    seg = (a("seg0"), a("seg1"), a("seg2"), a("seg3"))
    what = f"prompt_project_q + prompt_scan_paged {elem} ({B}, {S}, {D}) H {H} Hkv {Hkv}"
    assert mli.mli_launch_counts_reset() == 0
    assert mli.mli_prompt_project_q(a("table"), *seg, a("wq"), a("gathered"), a("q"), len(segs), 20, n_q, B, S, D, ELEM[elem], stream()) == 0
    arena.assert_guards_intact(what + ": projection")
    assert mli.mli_prompt_scan_paged(a("q"), a("table"), *seg, a("out"), len(segs), 20, n_q, B, S, D, H, Hkv, W, K, ELEM[elem], stream()) == 0
    arena.assert_guards_intact(what + ": scan")
    assert launches(mli, "gemm_f32_rows64" if elem == "f32" else "gemm_bf16_widened") == 1 and launches(mli, "scan_prompt") == 1
    q, out = f32(sf.bits(arena.view("q")), (n_q, D)), f32(sf.bits(arena.view("out")), (n_q, D))
    # (the projection's GEMM covers all n_q rows: a q row of no position is the product of whatever `gathered` held)
    assert (out[nobody] == SENTINEL).all(), f"{what}: a dense row of the output that belongs to no query was written"
    for name, got in (("q", q), ("out", out)):
        assert np.isfinite(got[where]).all() and (got[where] != SENTINEL).any(axis=1).all(), f"{what}: {name}"
    x = fm.gather_pages(values, c["table"], L, S, D, 0)[rows, pos].astype(np.float64)
    w64 = gm.decode(wq, "f32" if elem == "f32" else "bf16").astype(np.float64)
    bound = D * 2.0 ** -24 * (np.abs(x) @ np.abs(w64))
    worst = float((np.abs(q[where] - x @ w64) / bound).max())
    print(f"SCRATCH {what} | q: worst error {worst:.3e} of the bound D 2^-24 sum |x w|")
    assert worst <= 1.0
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    qv = np.ascontiguousarray(q[where])
    model = pm.model_prompt(qv, ktm, v_rows, rows, pos, H, Hkv, W, K)
    o_or = pm.oracle_prompt(oracle, qv, ktm, v_rows, rows, pos, H, Hkv, W, K)
    gqa.assert_within(gqa.compare(out[where], o_or, model, ("flat",) * H, what=what), what)
