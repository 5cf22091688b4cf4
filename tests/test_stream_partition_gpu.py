"""The equal-page-shares scan (csrc/attention_stream.hip) held to the float64 model on length vectors that place row
boundaries against share boundaries (tests/stream_model.py).  The attention arithmetic of this kernel
is covered by tests/test_attention_accuracy_gpu.py; what is covered here is the PARTITION -- the prefix sum of the page
counts, G, the static shares, the granules handed out by ticket, the row search, the count of triples a row waits for
and their slots, the groups of MAXSEG rows, empty rows inside a piece, waves without a page -- at the sizes that reach every
kernel variant.  tests/test_stream_model_cpu.py proves that the vectors reach every partition event on this chip's
G_launch and that the comparison made here fails for nine partition bugs.

Tolerance: the project's rule unchanged, max(8 x E_oracle, 16 x 2^-24), E_oracle from the fp32 CPU oracle's scan of the same
pages.  Dead slots are NaN.  Every launch is made twice and must give the same bits, leave the arrival counters and the
ticket at zero, write exact zeros for empty rows and leave no sentinel."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import f64_model as fm
import stream_model as sm
from accuracy_gpu import REPORT, SENTINEL, Checker, lean, lean_twice, paged_inputs
from gpu_util import host

pytestmark = pytest.mark.gpu

S = 1024                  # the kernel's minimum n_sequence
# name: (emb_dim, page types, vectors) -- the kernel variants of launch_stream_decode
#   D64    f32 NJ 1 / MAXSEG 4, bf16, fp8 RPI 4
#   D512   f32 NJ 2 / MAXSEG 4, fp8 RPI 2
#   D1024  bf16 NJ 2 / MAXSEG 2, fp8 RPI 1 / MAXSEG 2
SHAPES = {"D64": (64, ("f32", "bf16", "fp8"), tuple(sm.N_ARRAYS)), "D512": (512, ("f32", "fp8"), sm.SMALL_VECTORS),
          "D1024": (1024, ("bf16", "fp8"), sm.SMALL_VECTORS)}
PATH = "equal-page-shares scan, partition vectors"


def _families(name):
    return (("flat",) + (("early_peak", "late_peak") if name in sm.PEAK_VECTORS else ()) +
            (("offset-",) if name in sm.OFFSET_VECTORS else ()))


# one test per (shape, vector, array, family), the family varying fastest: the base case is built once per (shape, array)
CASES = [pytest.param(shape, name, k, family, id=f"{shape}-{name}{k}-{family}")
         for shape, (_, _, names) in SHAPES.items() for name in names for k in range(sm.N_ARRAYS[name])
         for family in _families(name)]


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("MLI_ACCURACY_REPORT")
    if path:
        with open(path, "w") as f:
            json.dump({" | ".join(k): v for k, v in sorted(REPORT.items())}, f, indent=1)


def _g_launch(dev):
    return 2 * torch.cuda.get_device_properties(dev).multi_processor_count


@functools.lru_cache(maxsize=1)
def _base(name, k, D, G_launch):
    L = sm.stream_vectors(G_launch, S)[name][k]
    return sm.vector_case(7200 + k, L, S, D)


def _tune_stream(mli, dyn, gran, stream=1, min_tokens=0):
    assert mli.mli_tune(b"scan_stream", stream) == 0
    assert mli.mli_tune(b"scan_stream_min_tokens", min_tokens) == 0
    assert mli.mli_tune(b"scan_stream_dynamic_pct", dyn) == 0
    assert mli.mli_tune(b"scan_stream_granule", gran) == 0


def _contract(ops, x, got, what):
    """What every launch owes besides the numbers."""
    ws, need = ops.workspace_for(x.B, x.S, x.D, x.q.device)
    assert need > 65536 and not host(ws[:65536]).any(), f"{what}: the arrival counters and the ticket are zero afterwards"
    assert not (got == SENTINEL).any(), f"{what}: rows {np.nonzero((got == SENTINEL).any(axis=1))[0][:8].tolist()} were not written"
    assert not got[x.lengths == 0].any(), f"{what}: rows of length 0 are exactly 0"


def _the_triples_are_those_of_the_restated_pieces(ops, x, dyn, gran, G_launch, tol_x, what):
    """The (m, l) statistics the launch left in its workspace, row by row and slot by slot, against the maxima of the
    restated pieces: |m - m^| within the score tolerance of the case (a maximum of fp32 scores is off by no more than a
    score is).  This is also what tells this kernel's launch from the chunked scan's, which the library takes silently
    where the equal-shares form does not apply: its statistics are those of 64-token chunks."""
    pt = sm.partition(x.lengths, S, G_launch, dyn, gran)
    want = sm.piece_maxima(x.model.x, x.lengths, pt)
    if not want:
        return
    ws, _ = ops.workspace_for(x.B, x.S, x.D, x.q.device)
    per_row = S // 64
    ml = host(ws[65536:65536 + x.B * per_row * 8]).view(np.float32).reshape(x.B, per_row, 2)
    worst = 0.0
    for b, m in want.items():
        assert len(m) == pt.row_pieces[b] <= per_row
        worst = max(worst, float(np.abs(ml[b, :len(m), 0].astype(np.float64) - np.asarray(m)).max()) / x.model.x_scale[b])
    print(f"TRIPLES {what}: {len(want)} rows, worst |m - m^| / scale {worst:.3e}  tol {tol_x:.3e}")
    assert worst <= tol_x, f"{what}: the workspace does not hold the maxima of the restated pieces ({worst:.3e} > {tol_x:.3e})"


@pytest.mark.parametrize("shape,name,k,family", CASES)
def test_partition_vectors(oracle, mli, dev, shape, name, k, family):
    from min_llm_inference_amd import ops
    D, elems, _ = SHAPES[shape]
    G_launch = _g_launch(dev)
    c = _base(name, k, D, G_launch)
    L = c["lengths"]
    if name in sm.SMALL_VECTORS:
        assert sm.page_counts(L, S).sum() <= 2048
    if family != "flat" and name != "tiny":     # (tiny: the arrays of P >= 31)
        assert any((sm.partition(L, S, G_launch, d, g).row_pieces >= 2).any() for d, g in sm.SPLITS)
    for elem in elems:
        if elem == "fp8":
            assert ops.has_fp8()
        ck = Checker(family, elem)
        x = paged_inputs(oracle, dev, c, family, elem, n_sequence=S)
        assert x.S == S and x.pool.numel() * x.pool.element_size() < 256 << 20
        e_o = fm.attention_error(x.oracle[2], x.model)
        tol_x = fm.tolerance(fm.score_error(x.oracle[0], x.model))
        try:
            for dyn, gran in sm.SPLITS:
                _tune_stream(mli, dyn, gran)
                what = f"{name}[{k}] {elem} {family}, {dyn} % in granules of {gran}"
                got = lean_twice(ops, x, elem, what)
                _contract(ops, x, got, what)
                ck.check(PATH, "attention", fm.attention_error(got, x.model), e_o)
                _the_triples_are_those_of_the_restated_pieces(ops, x, dyn, gran, G_launch, tol_x, what)
        finally:
            _tune_stream(mli, 4, 64, min_tokens=1 << 21)
        ck.done()


@pytest.mark.parametrize("name,k", [(n, k) for n in sm.N_ARRAYS for k in range(sm.N_ARRAYS[n])])
def test_the_chunked_lean_scan_on_the_same_vectors(oracle, mli, dev, name, k):
    """scan_stream = 0: the (row, chunk) grid on the same pages against the same model -- two implementations that agree
    with the truth on the same inputs."""
    from min_llm_inference_amd import ops
    c = _base(name, k, 64, _g_launch(dev))
    for elem in SHAPES["D64"][1]:
        ck = Checker("flat", elem)
        x = paged_inputs(oracle, dev, c, "flat", elem, n_sequence=S)
        try:
            _tune_stream(mli, 4, 64, stream=0)
            got = lean(ops, x, elem)
            _contract(ops, x, got, f"{name}[{k}] {elem}, chunked")
            ck.check("paged scan, lean, partition vectors", "attention", fm.attention_error(got, x.model),
                     fm.attention_error(x.oracle[2], x.model))
        finally:
            _tune_stream(mli, 4, 64, min_tokens=1 << 21)
        ck.done()
