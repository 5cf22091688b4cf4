"""The resident slice of the equal-page-shares scan (csrc/attention_stream.hip, mli_tune "scan_resident_mib"):
where the K/V stream is non-temporal, the pages whose address hashes under a threshold are loaded with the default cache
policy instead, so that they stay in the Infinity Cache from one decode step to the next.  Which policy a page is read
with changes no bit of the result: for every kernel variant, attention_result with a third of the pages kept, two thirds
and all of them is the bits of scan_resident_mib = 0.

The test restates the rule on the page table it built, through the two functions the library exports for that
(mli_scan_resident_threshold, mli_scan_resident_keeps): the kept count is 0, strictly between 0 and P twice, and P, so
both policies ran in the launches compared.  Inputs and the contract of a launch (twice the same bits, arrival counters
and ticket back at zero, empty rows exactly zero, no sentinel left) are those of tests/accuracy_gpu.py and
tests/test_stream_partition_gpu.py; dead slots are NaN."""
import functools

import numpy as np
import pytest

import stream_model as sm
from accuracy_gpu import ELEM, ESIZE, SENTINEL, lean_twice, paged_inputs
from gpu_util import host
from helpers import PAGE, assert_equal

pytestmark = pytest.mark.gpu

S = 1024                  # the kernel's minimum n_sequence
DEFAULT_MIB = 192         # the library's default for "scan_resident_mib"
# one per kernel variant of launch_stream_decode (tests/test_stream_partition_gpu.py), and the flagship's: D512 bf16
SHAPES = [(64, "f32"), (64, "bf16"), (64, "fp8"), (512, "f32"), (512, "bf16"), (512, "fp8"), (1024, "bf16"), (1024, "fp8")]


@functools.lru_cache(maxsize=1)
def _case(D, esize):
    """About 48 rows: the edge lengths and seeded random ones -- more where the pages are small, until the rows' K/V is
    3.2 MiB, so that whole MiB give a threshold near a third and near two thirds."""
    rng = np.random.default_rng(9100 + D)
    L = [0, 1, 15, 16, 17, S]
    kv = 2 * PAGE * D * esize
    while len(L) < 48 or sm.page_counts(L, S).sum() * kv < 3.2 * 2 ** 20:
        L.append(int(rng.integers(1, S + 1)))
    return sm.vector_case(9100 + D, np.asarray(L, np.int32), S, D)


def _contract(ops, x, got, what):
    ws, need = ops.workspace_for(x.B, x.S, x.D, x.q.device)
    assert need > 65536 and not host(ws[:65536]).any(), f"{what}: the arrival counters and the ticket are zero afterwards"
    assert not (got == SENTINEL).any(), f"{what}: rows {np.nonzero((got == SENTINEL).any(axis=1))[0][:8].tolist()} were not written"
    assert not got[x.lengths == 0].any(), f"{what}: rows of length 0 are exactly 0"


@pytest.mark.parametrize("D,elem", SHAPES, ids=[f"D{d}-{e}" for d, e in SHAPES])
def test_the_resident_slice_changes_no_bit(oracle, mli, dev, D, elem):
    from min_llm_inference_amd import ops
    if elem == "fp8":
        assert ops.has_fp8()
    c = _case(D, ESIZE[elem])
    x = paged_inputs(oracle, dev, c, "flat", elem, n_sequence=S)
    table = host(x.page_table)
    live = [int(table[b, i]) for b in range(x.B) for i in range(int(sm.page_counts(x.lengths, S)[b]))]
    P = len(live)
    assert P == sm.page_counts(x.lengths, S).sum() and all(live)
    total_mib = P * 2 * PAGE * D * ESIZE[elem] / 2 ** 20
    third, two_thirds, everything = max(1, round(total_mib / 3)), round(2 * total_mib / 3), int(total_mib) + 1
    assert third < two_thirds < everything <= 240

    def kept(mib):
        thr = mli.mli_scan_resident_threshold(P, D, ELEM[elem], mib)
        assert 0 <= thr <= 65536
        return thr, sum(mli.mli_scan_resident_keeps(p, thr) for p in live)

    try:
        assert mli.mli_tune(b"scan_stream", 1) == 0 and mli.mli_tune(b"scan_stream_min_tokens", 0) == 0
        assert mli.mli_tune(b"nt_loads", 1) == 0
        assert mli.mli_tune(b"scan_resident_mib", 0) == 0
        assert kept(0) == (0, 0)
        base = lean_twice(ops, x, elem, f"D{D} {elem}, nothing kept")
        _contract(ops, x, base, f"D{D} {elem}, nothing kept")
        counts = []
        for mib in (third, two_thirds, everything):
            thr, n = kept(mib)
            counts.append(n)
            what = f"D{D} {elem}, {mib} of {total_mib:.1f} MiB kept (threshold {thr}: {n} of {P} pages)"
            print("RESIDENT", what)
            assert mli.mli_tune(b"scan_resident_mib", mib) == 0
            got = lean_twice(ops, x, elem, what)
            _contract(ops, x, got, what)
            assert_equal(got, base, what=f"{what} against nothing kept")
        assert 0 < counts[0] < counts[1] < P and counts[2] == P, (counts, P)
        assert 0 < mli.mli_scan_resident_threshold(P, D, ELEM[elem], third) < mli.mli_scan_resident_threshold(P, D, ELEM[elem], two_thirds) < 65536
    finally:
        mli.mli_tune(b"scan_resident_mib", DEFAULT_MIB)
        mli.mli_tune(b"nt_loads", 2)
        mli.mli_tune(b"scan_stream_min_tokens", 1 << 21)
