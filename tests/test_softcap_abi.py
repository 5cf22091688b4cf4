"""The soft-capping entry points at the drop-in boundary, without a GPU: the symbols exist and are bound, the ABI version is
unchanged, one head, fp8 pages, a cap that is 0, negative, NaN or infinite, bad head counts and every unsupported shape are
refused before anything touches a device (null device pointers: validation precedes every GPU call) by both scans and both
compositions, accepted shapes get past the argument check (the refusal is then the workspace's), the launch families are known
and at zero, the capped prompt scan keeps mli_prompt_scan_tq (there is no second function), the headers compile as C99 and
C++17, a plain C host links against the library and calls one entry point, and the engine setter refuses a null handle."""
import ctypes
import os
import shutil
import subprocess

import pytest

from test_window_abi import BAD_HEADS, BAD_PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
SYMBOLS = ("mli_decode_scan_paged_softcap", "mli_paged_attention_lean_softcap", "mli_prompt_scan_paged_softcap",
           "mli_paged_prompt_logprobs_softcap", "mli_engine_set_softcap")
FORMS = ((0, 0), (-3, 0), (40, 0), (5, 0), (40, 4), (40, 20), (0, 4), (1000000, 4))     # (window, n_sink)
BAD_CAPS = (0.0, -0.0, -1.0, -50.0, float("nan"), float("inf"), -float("inf"))
PTR = ctypes.c_void_p(256)      # a non-null address nobody follows: every call here ends before a launch


def _scan(mli, B, S, D, H, Hkv, W, K, elem, cap=30.0):
    return mli.mli_decode_scan_paged_softcap(None, None, None, None, B, S, D, H, Hkv, W, K, cap, elem, None, 0, None)


def _lean(mli, B, S, D, H, Hkv, W, K, elem, cap=30.0, rope=None):
    return mli.mli_paged_attention_lean_softcap(None, None, None, None, None, None, None, None, B, S, D, 0, H, Hkv, W, K, cap, rope,
                                                elem, None, 0, None)


def _prompt(mli, B, S, D, H, Hkv, W, K, elem, cap=30.0, n_seg=1):
    """every pointer given: what is left to refuse the call is the shape, the heads and the cap"""
    return mli.mli_prompt_scan_paged_softcap(PTR, PTR, PTR, PTR, PTR, PTR, PTR, n_seg, 1, 1, B, S, D, H, Hkv, W, K, cap, elem, None)


def _score(mli, B, S, D, H, Hkv, W, K, elem, cap=30.0):
    return mli.mli_paged_prompt_logprobs_softcap(PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, PTR, None, None, 1, 1, 1, B, S, D, 64, H, Hkv,
                                                 W, K, cap, elem, 0, None, 0, None)


ALL = (_scan, _lean, _prompt, _score)


def test_symbols_are_exported_and_bound(mli):
    import inspect
    from min_llm_inference_amd import _lib, engine, ops
    for name in SYMBOLS:
        assert hasattr(mli, name), name
        assert name in _lib.SIGNATURES or name in _lib.ENGINE_SIGNATURES, name
    assert len(_lib.SIGNATURES["mli_decode_scan_paged_softcap"]) == 16
    assert len(_lib.SIGNATURES["mli_paged_attention_lean_softcap"]) == 22
    assert len(_lib.SIGNATURES["mli_prompt_scan_paged_softcap"]) == len(_lib.SIGNATURES["mli_prompt_scan_paged"]) + 1
    assert len(_lib.SIGNATURES["mli_paged_prompt_logprobs_softcap"]) == len(_lib.SIGNATURES["mli_paged_prompt_logprobs"]) + 1
    assert _lib.ENGINE_SIGNATURES["mli_engine_set_softcap"] == [ctypes.c_void_p, ctypes.c_float]
    assert mli.mli_abi_version() == 4          # no existing signature changed
    assert not hasattr(mli, "mli_prompt_scan_tq_softcap")        # the capped variants keep the queries per workgroup
    assert not hasattr(mli, "mli_attention_softcap_workspace_bytes")        # the workspace is the multi-head one
    for fn in (ops.decode_scan_paged_softcap, engine.Engine.set_softcap):
        assert callable(fn)
    for fn in (ops.paged_attention_lean, ops.prompt_scan_paged, ops.paged_prompt_logprobs):
        assert inspect.signature(fn).parameters["softcap"].default is None
    assert inspect.signature(engine.Engine.__init__).parameters["softcap"].default is None


def test_one_head_is_refused(mli):
    for elem in (F32, BF16, FP8):
        for S in (64, 1024):
            for W, K in FORMS:
                for call in ALL:
                    assert call(mli, 8, S, 128, 1, 1, W, K, elem) == BAD_ARG, (call.__name__, S, W, K, elem)


@pytest.mark.parametrize("H,Hkv", [(8, 4), (8, 1), (8, 8), (2, 1), (2, 2)])
def test_fp8_pages_bad_caps_and_negative_sinks_are_refused(mli, H, Hkv):
    for W, K in FORMS:
        for call in ALL:
            assert call(mli, 8, 64, 256, H, Hkv, W, K, FP8) == BAD_ARG, call.__name__
            assert call(mli, 8, 64, 256, H, Hkv, W, K, 3) == BAD_ARG, call.__name__
            for elem in (F32, BF16):
                for cap in BAD_CAPS:
                    assert call(mli, 8, 64, 256, H, Hkv, W, K, elem, cap=cap) == BAD_ARG, (call.__name__, cap)
                    assert call(mli, 8, 1024, 256, H, Hkv, W, K, elem, cap=cap) == BAD_ARG      # before any workspace is looked at
    for elem in (F32, BF16):
        for W in (0, 12, 64):
            for call in ALL:
                assert call(mli, 8, 64, 256, H, Hkv, W, -1, elem) == BAD_ARG, call.__name__
    assert _prompt(mli, 8, 64, 256, H, Hkv, 0, 0, F32, cap=0.0, n_seg=0) == BAD_ARG       # a bad cap beside nothing to do, too


@pytest.mark.parametrize("H,Hkv", [(8, 3), (8, 5), (8, 0), (8, -1), (8, 16), (8, 9), (6, 4), (2, 3), (1, 2), (1, 0), (0, 1), (0, 0),
                                   (-2, 1), (3, 2)])
def test_bad_head_counts_are_refused(mli, H, Hkv):
    for elem in (F32, BF16, FP8):
        for S in (64, 1024):
            for W, K in FORMS:
                for call in ALL:
                    assert call(mli, 8, S, 192 if H in (3, 6) else 256, H, Hkv, W, K, elem) == BAD_ARG, (call.__name__, S, W, K, elem)


@pytest.mark.parametrize("what,B,S,D,H,elem", BAD_HEADS + BAD_PLAIN, ids=[b[0] for b in BAD_HEADS + BAD_PLAIN])
def test_unsupported_shapes_are_refused_before_any_launch(mli, what, B, S, D, H, elem):
    """everything the heads / window entry points refuse, with every divisor of H as n_kv_heads, plain, windowed and with sinks"""
    for Hkv in [d for d in range(1, H + 1) if H % d == 0]:
        for W, K in ((0, 0), (12, 0), (12, 4), (S - 2, 1), (S, 0)):
            assert _scan(mli, B, S, D, H, Hkv, W, K, elem) == BAD_ARG, (Hkv, W, K)
            assert _lean(mli, B, S, D, H, Hkv, W, K, elem) == BAD_ARG, (Hkv, W, K)
            assert _lean(mli, B, S, D, H, Hkv, W, K, elem, rope=PTR) == BAD_ARG, (Hkv, W, K)


def test_accepted_shapes_get_past_the_argument_check(mli):
    """B 8, S 1024: several items per row, so the scan needs the workspace body and says so -- after the arguments passed.  The
    edges of the shape set: head_dim 32 and 256, fp32 pages to emb_dim 512, bf16 pages to 1024, every group size."""
    shapes = ((F32, 64, 2, 1), (F32, 512, 2, 2), (F32, 512, 16, 4), (F32, 192, 3, 1), (F32, 192, 6, 2), (F32, 256, 8, 8),
              (BF16, 1024, 4, 1), (BF16, 1024, 32, 8), (BF16, 1024, 16, 16), (BF16, 192, 6, 3), (BF16, 64, 2, 1), (BF16, 512, 8, 2))
    for elem, D, H, Hkv in shapes:
        for W, K in ((0, 0), (256, 0), (256, 4), (2000, 4), (256, 768)):
            for cap in (50.0, 1.0, 1e-3, 3e38):
                assert _scan(mli, 8, 1024, D, H, Hkv, W, K, elem, cap=cap) == WORKSPACE, (elem, D, H, Hkv, W, K, cap)
        assert _score(mli, 8, 1024, D, H, Hkv, 0, 0, elem) == WORKSPACE, (elem, D, H, Hkv)     # the scratch, after the arguments
    assert _scan(mli, 8, 1024, 1024, 4, 1, 0, 0, F32) == BAD_ARG          # fp32 rows of more than two lane loads
    assert _scan(mli, 8, 1024, 2048, 8, 1, 0, 0, BF16) == BAD_ARG
    assert _scan(mli, 8, 1024, 128, 8, 8, 0, 0, F32) == BAD_ARG           # head_dim 16
    assert _prompt(mli, 8, 64, 256, 8, 2, 0, 0, F32, n_seg=0) == 0        # no segments: nothing to do
    assert _prompt(mli, 8, 64, 256, 8, 2, 0, 0, F32, n_seg=-1) == BAD_ARG


def test_the_prompt_scan_keeps_its_queries_per_workgroup(mli):
    """mli_kernels.h: the capped variants run mli_prompt_scan_tq queries per workgroup -- 8 / 4 (fp32) and 4 / 2 (bf16)"""
    assert [mli.mli_prompt_scan_tq(D, 4, e) for D, e in ((128, F32), (512, F32), (256, BF16), (1024, BF16))] == [8, 4, 4, 2]


def test_the_launch_families_are_known_and_at_zero(mli):
    n = ctypes.c_ulonglong(99)
    assert mli.mli_launch_counts_reset() == 0
    for family in (b"scan_heads_softcap", b"scan_prompt_softcap"):
        assert mli.mli_launch_count(family, ctypes.byref(n)) == 0 and n.value == 0
    _scan(mli, 8, 1024, 256, 8, 2, 0, 0, BF16)                            # refused for its workspace: nothing was enqueued
    _scan(mli, 8, 64, 256, 1, 1, 0, 0, BF16)
    _prompt(mli, 8, 64, 256, 1, 1, 0, 0, BF16)
    for family in (b"scan_heads_softcap", b"scan_prompt_softcap", b"scan_heads_window", b"scan_heads_alibi", b"scan_prompt"):
        assert mli.mli_launch_count(family, ctypes.byref(n)) == 0 and n.value == 0, family


def test_the_engine_setter_refuses_a_null_handle(mli):
    for cap in (30.0, 0.0, -1.0, float("nan")):
        assert mli.mli_engine_set_softcap(None, cap) == -1
        assert b"null argument" in mli.mli_engine_last_error()


C_HOST = r"""
#include <math.h>
#include <stdio.h>
#include "mli_kernels.h"
#include "mli_engine.h"
int main(void) {
    int (*scan)(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, int, float, int, void*, size_t,
                void*) = mli_decode_scan_paged_softcap;
    int (*lean)(void* const*, const int*, const void*, const void*, const void*, const int*, float*, float*, int, int, int, int, int,
                int, int, int, float, const float*, int, void*, size_t, void*) = mli_paged_attention_lean_softcap;
    int (*prompt)(const float*, const void* const*, const int*, const int*, const int*, const int*, float*, int, int, int, int, int,
                  int, int, int, int, int, float, int, void*) = mli_prompt_scan_paged_softcap;
    int (*score)(const void* const*, const int*, const void*, const float*, const int*, const int*, const int*, const int*, float*,
                 int*, float*, int, int, int, int, int, int, int, int, int, int, int, float, int, int, void*, size_t, void*)
        = mli_paged_prompt_logprobs_softcap;
    int (*set)(mli_engine*, float) = mli_engine_set_softcap;
    (void)lean; (void)prompt; (void)score; (void)set;
    /* refusals are decided before anything touches a device: one head, then a cap that is not a number */
    if (scan(0, 0, 0, 0, 8, 64, 128, 1, 1, 0, 0, 30.0f, MLI_ELEM_F32, 0, 0, 0) != MLI_ERR_BAD_ARG) return 2;
    if (scan(0, 0, 0, 0, 8, 64, 128, 4, 2, 0, 0, (float)NAN, MLI_ELEM_F32, 0, 0, 0) != MLI_ERR_BAD_ARG) return 3;
    if (scan(0, 0, 0, 0, 8, 1024, 128, 4, 2, 0, 0, 30.0f, MLI_ELEM_BF16, 0, 0, 0) != MLI_ERR_WORKSPACE) return 4;
    puts("ok");
    return mli_abi_version() == 4 ? 0 : 1;
}
"""


def test_a_plain_c_host_compiles_against_the_headers_and_calls_an_entry_point(mli, tmp_path):
    src = tmp_path / "softcap.c"
    src.write_text(C_HOST)
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "min_llm_inference_amd", "lib")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    exe = tmp_path / "softcap_host"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lmli_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
