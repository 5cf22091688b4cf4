"""The projection, prefill and logits GEMMs against the float64 model of tests/gemm_model.py (GEMM block), at the
tile edges, k tails and dispatch thresholds of the launchers in csrc/proj_gemm.hip, proj_gemm_panel.hip and
proj_gemm_bf16.hip.  Every case calls a public entry point through ops, starts from random finite memory, and asserts
(a) every written q / K / V / logit within tolerance (fp32: f64_model.tolerance of the CPU oracle's error on the same
inputs, and the ceiling K * 2^-24; bf16 / fp8 stores: gemm_model.stored_error under the same tolerance), (b) every byte
the contract does not write is bit-identical to before, rows of length 0 included, (c) nothing non-finite.  The case ids
name the kernel the launcher picks for the shape and the mli_tune knobs of the case (profiles/gemm_edges_kernels.txt is
the list a kernel trace of this file shows).  tests/test_gemm_model_cpu.py proves that the judge can fail."""
import contextlib

import numpy as np
import pytest
import torch

import gemm_model as gm
from gpu_util import host

pytestmark = pytest.mark.gpu

# the defaults of tests/test_error_paths.py for the knobs the GEMM launchers read
DEFAULTS = {b"fill_compact": 1, b"latest_compact": 1, b"gemm_split": 1, b"gemm_bf16_split": 1, b"prefill_fused": 1,
            b"gemm_panel": 1, b"gemm_tall_tiles": 1, b"bf16_native_mfma": 1}
KNOB = {"fc": b"fill_compact", "lc": b"latest_compact", "split": b"gemm_split", "pf": b"prefill_fused", "panel": b"gemm_panel",
        "tall": b"gemm_tall_tiles", "native": b"bf16_native_mfma"}


@contextlib.contextmanager
def tuned(mli, knobs):
    try:
        for k, v in knobs.items():
            assert mli.mli_tune(KNOB[k], v) == 0, k
        yield
    finally:
        for k, v in DEFAULTS.items():
            mli.mli_tune(k, v)


def _t(a, dev):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint16:
        a = a.view(np.int16)
    return torch.from_numpy(a).to(dev)


def _shifted(a, dev):
    """The same float32 values at an address that is 4 bytes past a 16-byte boundary: what makes a launcher's aligned16()
    test fail and the scalar-load (non-VEC4) instantiation run."""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.zeros(a.size + 4, dtype=torch.float32, device=dev)
    view = buf[1:1 + a.size].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _weights(c, dev, shift):
    if c.fmt == "f32":
        return {n: (_shifted(w, dev) if shift else _t(w, dev)) for n, w in c.w.items()}
    return {n: _t(gm.encode(w, "bf16"), dev) for n, w in c.w.items()}   # bf16 bit patterns (int16 tensors)


def _run(oracle, mli, dev, label, built, knobs, shift=(), rule=True):
    """One case: build the device state, call the entry point of (layout, fmt, mode), judge what it left."""
    from min_llm_inference_amd import ops
    c, mode = built
    fmt = c.fmt
    e = gm.Expect(oracle, c, mode)
    w = _weights(c, dev, "w" in shift)
    L, new_idx = _t(c.L, dev), _t(c.new_idx, dev)
    q = _t(c.q, dev)
    pre = {}
    if mode == "prefill":
        pre = {"emb": _shifted(c.emb, dev) if "emb" in shift else _t(c.emb, dev),
               "wpe": _shifted(c.wpe, dev) if "emb" in shift else _t(c.wpe, dev), "tok": _t(c.tok, dev)}
    fig = gm.Figures(label)
    also = ()
    with tuned(mli, knobs):
        if c.layout == "paged":
            pool = _t(c.pool, dev)
            assert pool.data_ptr() % 16 == 0
            table = _t(np.where(c.table >= 0, pool.data_ptr() + gm.ESIZE[fmt] * c.table, 0).astype(np.int64), dev)
            if mode == "latest":
                if fmt == "f32":
                    ops.launch_get_latest_k_q_v_paged_attention(table, L, w["wk"], w["wq"], w["wv"], q, c.S)
                elif fmt == "bf16":
                    ops.launch_get_latest_k_q_v_paged_attention_bf16(table, L, w["wk"], w["wq"], w["wv"], q, c.S)
                else:
                    ops.get_latest_k_q_v_paged_lean(table, L, w["wk"], w["wq"], w["wv"], q, c.S, elem=ops.ELEM_FP8)
            elif mode == "fill" and fmt == "fp8":
                # the fp8 fill without the encoder has no entry point of its own: the lean composition runs fill, latest
                # and the scan (whose output is not looked at); fill and latest are judged by their own Expect
                out = torch.zeros(c.B, c.Din, device=dev)
                ops.paged_attention_lean(table, L, w["wk"], w["wq"], w["wv"], new_idx, q, out, c.n_new, c.S, elem=ops.ELEM_FP8)
                e2 = gm.Expect(oracle, c, "latest")
                gm.judge(fig, c, e2, {"pool": host(pool)}, host(q), rule, also=e.rows)
                also = e2.rows
            elif mode == "fill":
                fn = ops.launch_fill_new_k_v_cache_paged_attention if fmt == "f32" else ops.launch_fill_new_k_v_cache_paged_attention_bf16
                fn(table, new_idx, L, w["wk"], w["wv"], c.n_new, c.S)
            else:
                ops.paged_prefill(pre["emb"], pre["wpe"], pre["tok"], table, L, new_idx, w["wk"], w["wv"], c.n_new, elem=gm.ELEM[fmt])
            after = {"pool": host(pool).view(gm.BITS[fmt]) if fmt == "bf16" else host(pool)}
        else:
            inp = _shifted(c.inp, dev) if "inp" in shift else _t(c.inp, dev)
            kt, v = _t(c.kt, dev), _t(c.v, dev)
            if mode == "latest":
                ops.launch_get_latest_kt_q_v(inp, L, w["wk"], w["wq"], w["wv"], kt, v, q)
            elif mode == "fill":
                ops.launch_fill_new_kt_v_cache(inp, new_idx, L, w["wk"], w["wv"], kt, v, c.n_new)
            else:
                ops.prefill(pre["emb"], pre["wpe"], pre["tok"], inp, L, new_idx, w["wk"], w["wv"], kt, v, c.n_new)
            after = {"kt": host(kt), "v": host(v)}
            if mode == "prefill":
                after["inp"] = host(inp)
    assert (host(L) == c.L).all() and (host(new_idx) == c.new_idx).all()
    if not (mode == "fill" and fmt == "fp8"):
        assert (host(q).view(np.uint32) == c.q.view(np.uint32)).all() or mode == "latest", "a fill wrote q_output"
    gm.judge(fig, c, e, after, host(q) if mode == "latest" else None, rule, also=also).done()


def _ids(cases):
    return [pytest.param(*c[1:], id=c[0]) for c in cases]


# ---- fp32 pages: projection ----------------------------------------------------------------------------------------------
# the four kernels a vec4 projection can take, by knobs: panel | 128-row tiles (MT 2) | 64-row tiles, loader / MFMA wave split
# from K 256 on (SPLIT) | 64-row tiles unsplit
PANEL = {"panel": 2}
TALL = {"panel": 0, "tall": 2}
TILED = {"panel": 0, "tall": 0, "split": 1}
UNSPLIT = {"panel": 0, "tall": 0, "split": 0}


def _f32_latest_cases():
    out, seed = [], 100
    for B, D in [(1, 4), (65, 60), (64, 64), (129, 68), (65, 252), (129, 256), (65, 260), (64, 516), (129, 516)]:
        split = "split" if D >= 256 else "vec4"
        for name, knobs in ((f"panel-B{B}-D{D}", PANEL), (f"mt2-compact-B{B}-D{D}", dict(TALL, lc=2)),
                            (f"{split}-dense-B{B}-D{D}", dict(TILED, lc=0)), (f"vec4-compact-B{B}-D{D}", dict(UNSPLIT, lc=2))):
            seed += 1
            out.append((name, seed, "signed", B, 48, D, knobs, ()))
    out += [("mt2-dense-B129-D260-positive", 150, "positive", 129, 32, 260, dict(TALL, lc=0), ()),
            ("panel-B65-D68-positive", 151, "positive", 65, 32, 68, PANEL, ()),
            ("split-compact-B65-D516-positive", 152, "positive", 65, 32, 516, dict(TILED, lc=2), ()),
            # default dispatch on either side of gemm_panel_wanted (K <= 512 and < 256 tiles of 64 x 64 over 3 D columns)
            ("default-panel-B65-D512", 153, "signed", 65, 32, 512, {}, ()),
            ("default-split-B65-D516", 154, "signed", 65, 32, 516, {}, ()),
            ("default-panel-240tiles-B1024-D320", 155, "signed", 1024, 32, 320, {}, ()),
            ("default-split-256tiles-B1024-D324", 156, "signed", 1024, 32, 324, {}, ()),
            # kMaxCompactRows: the live-row list up to 2048 rows, dense rows beyond
            ("vec4-compact-B2048-D64", 157, "signed", 2048, 32, 64, dict(UNSPLIT, lc=2), ()),
            ("vec4-compact-falls-back-B2049-D64", 158, "signed", 2049, 32, 64, dict(UNSPLIT, lc=2), ()),
            # weights one float off a 16-byte boundary: the scalar-load instantiation
            ("scalar-unaligned-w-B65-D68", 159, "signed", 65, 48, 68, {}, ("w",)),
            ("scalar-unaligned-w-compact-B129-D260", 160, "signed", 129, 32, 260, {"lc": 2}, ("w",))]
    return out


@pytest.mark.parametrize("seed,family,B,S,D,knobs,shift", _ids(_f32_latest_cases()))
def test_f32_paged_projection(oracle, mli, dev, request, seed, family, B, S, D, knobs, shift):
    _run(oracle, mli, dev, f"f32-latest:{request.node.callspec.id}", gm.latest_case(seed, "f32", family, B, S, D), knobs, shift)


# ---- fp32 pages: fill and prefill ----------------------------------------------------------------------------------------
def _f32_fill_cases():
    out, seed = [], 200
    for D in (4, 60, 64, 68, 252, 256, 260, 516):
        kern = "split" if D >= 256 else "vec4"
        for fc in (1, 0):
            seed += 1
            out.append((f"{kern}-{'flat' if fc else 'per-row'}-D{D}", seed, "signed", 12, 80, D, {"fc": fc}, (), "fill", None))
        if D >= 256:
            seed += 1
            out.append((f"vec4-flat-D{D}", seed, "signed", 12, 80, D, {"split": 0}, (), "fill", None))
    out += [("vec4-flat-B1-D68", 230, "signed", 1, 80, 68, {}, (), "fill", None),
            ("split-per-row-B1-D260", 231, "signed", 1, 144, 260, {"fc": 0}, (), "fill", None),
            ("vec4-flat-D60-positive", 232, "positive", 12, 80, 60, {}, (), "fill", None),
            ("split-flat-D516-positive", 233, "positive", 12, 80, 516, {}, (), "fill", None),
            ("vec4-flat-2048-new-rows-D8", 234, "signed", 2048, 16, 8, {}, (), "fill", np.ones(2048, np.int32)),
            ("vec4-flat-falls-back-2049-new-rows-D8", 235, "signed", 2049, 16, 8, {}, (), "fill", np.ones(2049, np.int32)),
            ("scalar-unaligned-w-flat-D68", 236, "signed", 12, 80, 68, {}, ("w",), "fill", None),
            ("scalar-unaligned-w-per-row-D260", 237, "signed", 12, 80, 260, {"fc": 0}, ("w",), "fill", None)]
    for D in (68, 260, 516):
        out.append((f"prologue-D{D}", 240 + D, "signed", 12, 80, D, {"pf": 2}, (), "prefill", None))
        out.append((f"encoder-then-fill-D{D}", 250 + D, "signed", 12, 80, D, {"pf": 0}, (), "prefill", None))
    out += [("prologue-scalar-unaligned-emb-D68", 260, "signed", 12, 80, 68, {"pf": 2}, ("emb",), "prefill", None),
            ("prologue-scalar-unaligned-w-D260", 261, "signed", 12, 80, 260, {"pf": 2}, ("w",), "prefill", None)]
    return out


@pytest.mark.parametrize("seed,family,B,S,D,knobs,shift,mode,lengths", _ids(_f32_fill_cases()))
def test_f32_paged_fill_and_prefill(oracle, mli, dev, request, seed, family, B, S, D, knobs, shift, mode, lengths):
    built = gm.fill_case(seed, "f32", family, B, S, D, mode=mode, lengths=lengths)
    _run(oracle, mli, dev, f"f32-{mode}:{request.node.callspec.id}", built, knobs, shift)


# ---- contiguous layout (transposed K) ------------------------------------------------------------------------------------
def _naive_cases():
    out, seed = [], 300
    for (Din, Dout), B, S in [((101, 257), 1, 100), ((101, 257), 65, 128), ((64, 68), 1, 128), ((64, 68), 65, 100),
                              ((260, 64), 1, 100), ((260, 64), 65, 128)]:
        shape = f"{Din}x{Dout}-B{B}-S{S}"
        variants = [("scalar", {})] if Din % 4 else [("panel", PANEL), ("mt2", dict(TALL, lc=2)), ("tiled", dict(TILED, lc=0))]
        for name, knobs in variants:
            seed += 1
            out.append((f"latest-{name}-{shape}", seed, Din, Dout, B, S, knobs, (), "latest"))
    for (Din, Dout), S in [((101, 257), 100), ((64, 68), 128), ((260, 64), 100)]:
        for fc in (1, 0):
            seed += 1
            out.append((f"fill-{'flat' if fc else 'per-row'}-{Din}x{Dout}-S{S}", seed, Din, Dout, 12, S, {"fc": fc}, (), "fill"))
        for pf in (2, 0):
            seed += 1
            # (the encoder kernel moves float4: a width that is no multiple of 4 takes the prologue form under either setting --
            # mli_prefill used to answer MLI_ERR_BAD_ARG there once "prefill_fused" or a width beyond 512 asked for two launches)
            form = "prologue" if pf else ("encoder-then-fill" if Din % 4 == 0 else "two-launches-asked-prologue-runs")
            out.append((f"prefill-{form}-{Din}x{Dout}-S{S}", seed, Din, Dout, 12, S, {"pf": pf}, (), "prefill"))
    out += [("latest-scalar-unaligned-inp-64x68-B65-S100", 340, 64, 68, 65, 100, {}, ("inp",), "latest"),
            ("latest-scalar-unaligned-w-260x64-B65-S100", 341, 260, 64, 65, 100, {}, ("w",), "latest"),
            ("fill-scalar-unaligned-w-64x68-S100", 342, 64, 68, 12, 100, {}, ("w",), "fill"),
            ("prefill-scalar-unaligned-emb-64x68-S100", 343, 64, 68, 12, 100, {"pf": 2}, ("emb",), "prefill"),
            ("prefill-default-wide-odd-prologue-517x64-S100", 344, 517, 64, 12, 100, {}, (), "prefill"),
            ("prefill-default-wide-encoder-then-fill-516x64-S100", 345, 516, 64, 12, 100, {}, (), "prefill")]
    return out


@pytest.mark.parametrize("seed,Din,Dout,B,S,knobs,shift,mode", _ids(_naive_cases()))
def test_contiguous_projection_fill_and_prefill(oracle, mli, dev, request, seed, Din, Dout, B, S, knobs, shift, mode):
    if mode == "latest":
        built = gm.latest_case(seed, "f32", "signed", B, S, Din, layout="naive", Dout=Dout)
    else:
        built = gm.fill_case(seed, "f32", "signed", B, S, Din, layout="naive", Dout=Dout, mode=mode)
    _run(oracle, mli, dev, f"naive-{mode}:{request.node.callspec.id}", built, knobs, shift)


# ---- bf16 pages ----------------------------------------------------------------------------------------------------------
def _deep(D):
    return "kb128" if 256 <= D <= 1024 else "kb32"


def _bf16_cases():
    out, seed = [], 400
    for B, D in [(1, 8), (65, 56), (64, 64), (129, 72), (65, 248), (129, 256), (65, 264), (64, 1024), (65, 1032)]:
        for name, knobs in ((f"latest-native-{_deep(D)}-compact-B{B}-D{D}", {"tall": 0, "lc": 2}),
                            (f"latest-native-mt2-kb64-dense-B{B}-D{D}", {"tall": 2, "lc": 0}),
                            (f"latest-widened-compact-B{B}-D{D}", {"native": 0, "lc": 2})):
            seed += 1
            out.append((name, seed, "signed", B, 48, D, knobs, "latest"))
    out += [("latest-native-mt2-kb64-compact-B129-D264", 430, "signed", 129, 32, 264, {"tall": 2, "lc": 2}, "latest"),
            ("latest-native-kb128-dense-B129-D256", 431, "signed", 129, 32, 256, {"tall": 0, "lc": 0}, "latest"),
            ("latest-native-kb32-B129-D72-positive", 432, "positive", 129, 32, 72, {"tall": 0}, "latest"),
            ("latest-native-mt2-kb64-B65-D248-positive", 433, "positive", 65, 32, 248, {"tall": 2}, "latest"),
            # default dispatch around the LDS-DMA kernel's range: D >= 1536, or D >= 1024 from 320 rows
            ("latest-default-tiled-B319-D1024", 434, "signed", 319, 32, 1024, {}, "latest"),
            ("latest-default-dma-B320-D1024", 435, "signed", 320, 32, 1024, {}, "latest"),
            ("latest-default-dma-B1-D1536", 436, "signed", 1, 32, 1536, {}, "latest"),
            ("latest-default-dma-B129-D1600", 437, "signed", 129, 32, 1600, {}, "latest"),
            ("latest-default-dma-B130-D1664", 438, "signed", 130, 32, 1664, {}, "latest"),
            ("latest-default-tiled-B64-D1472", 439, "signed", 64, 32, 1472, {}, "latest")]
    seed = 450
    for D in (8, 56, 64, 72, 248, 256, 264, 1024, 1032):
        seed += 1
        fc = seed % 2
        out.append((f"fill-native-kb32-{'flat' if fc else 'per-row'}-D{D}", seed, "signed", 12, 80, D, {"fc": fc}, "fill"))
    out += [("fill-native-kb32-flat-D72", 470, "signed", 12, 80, 72, {"fc": 1}, "fill"),
            ("fill-native-kb32-per-row-D264", 471, "signed", 12, 80, 264, {"fc": 0}, "fill"),
            ("fill-widened-flat-D72", 472, "signed", 12, 80, 72, {"native": 0}, "fill"),
            ("fill-widened-per-row-D264", 473, "signed", 12, 80, 264, {"native": 0, "fc": 0}, "fill"),
            ("fill-native-kb32-flat-D56-positive", 474, "positive", 12, 80, 56, {}, "fill"),
            ("prefill-prologue-D520", 475, "signed", 12, 80, 520, {"pf": 2}, "prefill"),
            ("prefill-encoder-then-fill-D256", 476, "signed", 12, 80, 256, {"pf": 0}, "prefill"),
            ("prefill-prologue-D72", 477, "signed", 12, 80, 72, {}, "prefill")]
    return out


@pytest.mark.parametrize("seed,family,B,S,D,knobs,mode", _ids(_bf16_cases()))
def test_bf16_paged(oracle, mli, dev, request, seed, family, B, S, D, knobs, mode):
    built = gm.latest_case(seed, "bf16", family, B, S, D) if mode == "latest" else gm.fill_case(seed, "bf16", family, B, S, D, mode=mode)
    _run(oracle, mli, dev, f"bf16-{mode}:{request.node.callspec.id}", built, knobs)


# ---- fp8 pages -----------------------------------------------------------------------------------------------------------
def _fp8_cases():
    out, seed = [], 500
    for B, D in [(1, 16), (65, 48), (129, 64), (200, 80), (65, 256), (129, 272), (200, 1024), (65, 1040)]:
        for name, knobs in ((f"latest-{_deep(D)}-compact-B{B}-D{D}", {"tall": 0, "lc": 2}),
                            (f"latest-mt2-kb64-dense-B{B}-D{D}", {"tall": 2, "lc": 0}),
                            (f"latest-mt2-kb64-compact-B{B}-D{D}", {"tall": 2, "lc": 2})):
            seed += 1
            out.append((name, seed, "signed", B, 48, D, knobs, "latest"))
    out += [("latest-kb128-dense-B200-D272-positive", 530, "positive", 200, 32, 272, {"tall": 0, "lc": 0}, "latest"),
            ("latest-mt2-kb64-B129-D80-positive", 531, "positive", 129, 32, 80, {"tall": 2}, "latest")]
    seed = 540
    for D in (16, 48, 64, 80, 256, 272, 1024, 1040):
        seed += 1
        out.append((f"fill-latest-scan-flat-D{D}", seed, "signed", 12, 80, D, {}, "fill"))
        seed += 1
        out.append((f"prefill-saturating-D{D}", seed, "signed", 12, 80, D, {}, "prefill"))
    out += [("fill-latest-scan-per-row-D48", 560, "signed", 12, 80, 48, {"fc": 0}, "fill"),
            ("fill-latest-scan-per-row-mt2-D272", 561, "signed", 12, 80, 272, {"fc": 0, "tall": 2, "lc": 2}, "fill"),
            ("prefill-per-row-D80", 562, "signed", 12, 80, 80, {"fc": 0}, "prefill")]
    return out


@pytest.mark.parametrize("seed,family,B,S,D,knobs,mode", _ids(_fp8_cases()))
def test_fp8_paged(oracle, mli, dev, request, seed, family, B, S, D, knobs, mode):
    from min_llm_inference_amd import ops
    assert ops.has_fp8()
    if mode == "latest":
        built = gm.latest_case(seed, "fp8", family, B, S, D)
    else:
        built = gm.fill_case(seed, "fp8", family, B, S, D, mode=mode, saturate=mode == "prefill")
    if mode == "prefill":   # one new row's x is beyond the format's range: it is stored, and multiplied, as +-448
        e = gm.Expect(None, built[0], mode)
        assert np.abs(e.x).max() == 448 and (np.abs(e.x) == 448).sum() >= D // 8
    _run(oracle, mli, dev, f"fp8-{mode}:{request.node.callspec.id}", built, knobs)


# ---- logits and the greedy head ------------------------------------------------------------------------------------------
def _logits_cases():
    out, seed = [], 600
    for B, V, D in [(1, 1, 4), (33, 31, 36), (65, 32, 252), (129, 33, 256), (33, 63, 260), (65, 64, 512), (129, 65, 516),
                    (33, 1030, 36), (65, 1030, 260)]:
        split = "split" if D >= 256 else "vec4"
        for name, knobs in ((f"panel-B{B}-V{V}-D{D}", PANEL), (f"mt2-B{B}-V{V}-D{D}", TALL), (f"{split}-B{B}-V{V}-D{D}", TILED),
                            (f"vec4-unsplit-B{B}-V{V}-D{D}", UNSPLIT)):
            seed += 1
            out.append((name, seed, "signed", B, V, D, knobs, ()))
    out += [("default-panel-240tiles-B1024-V960-D64", 640, "signed", 1024, 960, 64, {}, ()),
            ("default-vec4-256tiles-B1024-V1024-D64", 641, "signed", 1024, 1024, 64, {}, ()),
            ("panel-B65-V33-D36-positive", 642, "positive", 65, 33, 36, PANEL, ()),
            ("split-B129-V1030-D260-positive", 643, "positive", 129, 1030, 260, TILED, ()),
            ("scalar-unaligned-emb-B65-V33-D36", 644, "signed", 65, 33, 36, {}, ("emb",)),
            ("scalar-unaligned-att-B129-V65-D260", 645, "signed", 129, 65, 260, {}, ("att",))]
    return out


@pytest.mark.parametrize("seed,family,B,V,D,knobs,shift", _ids(_logits_cases()))
def test_logits_and_greedy_head(oracle, mli, dev, request, seed, family, B, V, D, knobs, shift):
    """launch_decoder's emb_score through the projection metric; decoder_fused's token against the float64 argmax."""
    from min_llm_inference_amd import ops
    # (a shifted emb_table is a contract of the GEMM's loads only: the head's own float4 read of the winning row is kept
    # out of that case by letting every row finish on its length)
    c = gm.LogitsCase(seed, family, B, V, D, finish="emb" in shift)
    att = _shifted(c.att, dev) if "att" in shift else _t(c.att, dev)
    emb = _shifted(c.emb, dev) if "emb" in shift else _t(c.emb, dev)
    wpe = _t(c.wpe, dev)
    fig = gm.Figures(f"logits:{request.node.callspec.id}")
    got = {}
    with tuned(mli, knobs):
        for head in ("unfused", "fused"):
            inp, L = _t(c.inp, dev), _t(c.L, dev)
            res = torch.full((B,), 77, dtype=torch.int32, device=dev)
            if head == "unfused":
                score = _t(c.score0, dev)
                ops.launch_decoder(att, emb, score, wpe, inp, L, res)
                got["score"] = host(score)
            else:
                ops.decoder_fused(att, emb, wpe, inp, L, res)
            got[head] = host(res).copy()
            # (b) the head writes the next embedding at position L of a live row that goes on, and nothing else
            after, tok = host(inp), got[head]
            fig.require(np.isfinite(after).all(), f"{head}: non-finite value in inp_embedding")
            mask = np.zeros(c.inp.shape, bool)
            for b in range(B):
                if c.L[b] > 0 and c.L[b] + 1 < c.S and 0 <= tok[b] < V and tok[b] != ops.EOF_TOKEN_ID:
                    mask[b, c.L[b]] = True
                    fig.require((after[b, c.L[b]] == c.emb[tok[b]] + c.wpe[c.L[b]]).all(), f"{head}: next embedding of row {b}")
            same = after.view(np.uint32)[~mask] == c.inp.view(np.uint32)[~mask]
            fig.require(same.all(), f"{head}: {int((~same).sum())} inp_embedding elements outside the next positions changed")
    gm.judge_logits(fig, oracle, c, got["score"], got["fused"], got["unfused"])
    fig.done()
