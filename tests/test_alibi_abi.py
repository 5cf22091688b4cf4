"""The ALiBi entry points at the drop-in boundary, without a GPU: the symbols exist and are bound, the ABI version is unchanged,
one head, fp8 pages, null slopes, bad head counts and every unsupported shape are refused before anything touches a device
(null device pointers: validation precedes every GPU call), accepted shapes get past the argument check (the refusal is then
the workspace's), the launch family is known and at zero, the headers compile as C99 and C++17, and the engine setter refuses
a null handle."""
import ctypes
import os
import shutil
import subprocess

import pytest

from test_window_abi import BAD_HEADS, BAD_PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
SYMBOLS = ("mli_decode_scan_paged_alibi", "mli_paged_attention_lean_alibi", "mli_alibi_slopes", "mli_engine_set_alibi")
FORMS = ((0, 0), (-3, 0), (40, 0), (5, 0), (40, 4), (40, 20), (0, 4), (1000000, 4))     # (window, n_sink)
SLOPES = ctypes.c_void_p(256)      # a non-null address nobody follows: every call here ends before a launch


def _scan(mli, B, S, D, H, Hkv, W, K, elem, slopes=SLOPES):
    return mli.mli_decode_scan_paged_alibi(None, None, None, None, B, S, D, H, Hkv, W, K, slopes, elem, None, 0, None)


def _lean(mli, B, S, D, H, Hkv, W, K, elem, slopes=SLOPES):
    return mli.mli_paged_attention_lean_alibi(None, None, None, None, None, None, None, None, B, S, D, 0, H, Hkv, W, K, slopes, elem,
                                              None, 0, None)


def test_symbols_are_exported_and_bound(mli):
    from min_llm_inference_amd import _lib, engine, ops
    for name in SYMBOLS:
        assert hasattr(mli, name), name
        assert name in _lib.SIGNATURES or name in _lib.ENGINE_SIGNATURES, name
    assert len(_lib.SIGNATURES["mli_decode_scan_paged_alibi"]) == 16
    assert len(_lib.SIGNATURES["mli_paged_attention_lean_alibi"]) == 21
    assert len(_lib.SIGNATURES["mli_alibi_slopes"]) == 2 and len(_lib.ENGINE_SIGNATURES["mli_engine_set_alibi"]) == 3
    assert mli.mli_abi_version() == 4          # no existing signature changed
    for fn in (ops.alibi_slopes, ops.decode_scan_paged_alibi, engine.Engine.set_alibi):
        assert callable(fn)
    import inspect
    assert "alibi_slopes" in inspect.signature(ops.paged_attention_lean).parameters
    assert "alibi" in inspect.signature(engine.Engine.__init__).parameters


def test_one_head_is_refused(mli):
    for elem in (F32, BF16, FP8):
        for S in (64, 1024):
            for W, K in FORMS:
                assert _scan(mli, 8, S, 128, 1, 1, W, K, elem) == BAD_ARG, (S, W, K, elem)
                assert _lean(mli, 8, S, 128, 1, 1, W, K, elem) == BAD_ARG, (S, W, K, elem)


@pytest.mark.parametrize("H,Hkv", [(8, 4), (8, 1), (8, 8), (2, 1), (2, 2)])
def test_fp8_pages_null_slopes_and_negative_sinks_are_refused(mli, H, Hkv):
    for W, K in FORMS:
        assert _scan(mli, 8, 64, 256, H, Hkv, W, K, FP8) == BAD_ARG
        assert _lean(mli, 8, 64, 256, H, Hkv, W, K, FP8) == BAD_ARG
        assert _scan(mli, 8, 64, 256, H, Hkv, W, K, 3) == BAD_ARG
        for elem in (F32, BF16):
            assert _scan(mli, 8, 64, 256, H, Hkv, W, K, elem, slopes=None) == BAD_ARG
            assert _lean(mli, 8, 64, 256, H, Hkv, W, K, elem, slopes=None) == BAD_ARG
            assert _scan(mli, 8, 1024, 256, H, Hkv, W, K, elem, slopes=None) == BAD_ARG      # before the workspace is looked at
    for elem in (F32, BF16):
        for W in (0, 12, 64):
            assert _scan(mli, 8, 64, 256, H, Hkv, W, -1, elem) == BAD_ARG
            assert _lean(mli, 8, 64, 256, H, Hkv, W, -1, elem) == BAD_ARG


@pytest.mark.parametrize("H,Hkv", [(8, 3), (8, 5), (8, 0), (8, -1), (8, 16), (8, 9), (6, 4), (2, 3), (1, 2), (1, 0), (0, 1), (0, 0),
                                   (-2, 1), (3, 2)])
def test_bad_head_counts_are_refused(mli, H, Hkv):
    for elem in (F32, BF16, FP8):
        for S in (64, 1024):
            for W, K in FORMS:
                assert _scan(mli, 8, S, 192 if H in (3, 6) else 256, H, Hkv, W, K, elem) == BAD_ARG, (S, W, K, elem)
                assert _lean(mli, 8, S, 192 if H in (3, 6) else 256, H, Hkv, W, K, elem) == BAD_ARG, (S, W, K, elem)


@pytest.mark.parametrize("what,B,S,D,H,elem", BAD_HEADS + BAD_PLAIN, ids=[b[0] for b in BAD_HEADS + BAD_PLAIN])
def test_unsupported_shapes_are_refused_before_any_launch(mli, what, B, S, D, H, elem):
    """everything the heads / window entry points refuse, with every divisor of H as n_kv_heads, plain, windowed and with sinks"""
    for Hkv in [d for d in range(1, H + 1) if H % d == 0]:
        for W, K in ((0, 0), (12, 0), (12, 4), (S - 2, 1), (S, 0)):
            assert _scan(mli, B, S, D, H, Hkv, W, K, elem) == BAD_ARG, (Hkv, W, K)
            assert _lean(mli, B, S, D, H, Hkv, W, K, elem) == BAD_ARG, (Hkv, W, K)


def test_accepted_shapes_get_past_the_argument_check(mli):
    """B 8, S 1024: several items per row, so the scan needs the workspace body and says so -- after the arguments passed.  The
    edges of the shape set: head_dim 32 and 256, fp32 pages to emb_dim 512, bf16 pages to 1024, every group size."""
    shapes = ((F32, 64, 2, 1), (F32, 512, 2, 2), (F32, 512, 16, 4), (F32, 192, 3, 1), (F32, 192, 6, 2), (F32, 256, 8, 8),
              (BF16, 1024, 4, 1), (BF16, 1024, 32, 8), (BF16, 1024, 16, 16), (BF16, 192, 6, 3), (BF16, 64, 2, 1), (BF16, 512, 8, 2))
    for elem, D, H, Hkv in shapes:
        for W, K in ((0, 0), (256, 0), (256, 4), (2000, 4), (256, 768)):
            assert _scan(mli, 8, 1024, D, H, Hkv, W, K, elem) == WORKSPACE, (elem, D, H, Hkv, W, K)
    assert _scan(mli, 8, 1024, 1024, 4, 1, 0, 0, F32) == BAD_ARG          # fp32 rows of more than two lane loads
    assert _scan(mli, 8, 1024, 2048, 8, 1, 0, 0, BF16) == BAD_ARG
    assert _scan(mli, 8, 1024, 128, 8, 8, 0, 0, F32) == BAD_ARG           # head_dim 16
    assert not hasattr(mli, "mli_attention_alibi_workspace_bytes")        # the workspace is the multi-head one


def test_the_launch_family_is_known_and_at_zero(mli):
    n = ctypes.c_ulonglong(99)
    assert mli.mli_launch_counts_reset() == 0
    assert mli.mli_launch_count(b"scan_heads_alibi", ctypes.byref(n)) == 0 and n.value == 0
    _scan(mli, 8, 1024, 256, 8, 2, 0, 0, BF16)                            # refused for its workspace: nothing was enqueued
    _scan(mli, 8, 64, 256, 1, 1, 0, 0, BF16)
    assert mli.mli_launch_count(b"scan_heads_alibi", ctypes.byref(n)) == 0 and n.value == 0
    assert mli.mli_launch_count(b"scan_heads_window", ctypes.byref(n)) == 0 and n.value == 0


def test_the_engine_setter_refuses_a_null_handle(mli):
    import numpy as np
    slopes = np.full(4, 0.5, np.float32)
    for ptr, n in ((None, 0), (slopes.ctypes.data_as(ctypes.c_void_p), 4)):
        assert mli.mli_engine_set_alibi(None, ptr, n) == -1
        assert b"null argument" in mli.mli_engine_last_error()


def test_headers_still_compile_as_c99_and_cxx17(tmp_path):
    src = tmp_path / "alibi.c"
    src.write_text('#include "mli_kernels.h"\n#include "mli_engine.h"\n'
                   "int main(void) {\n"
                   "    int (*scan)(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, int, const float*,\n"
                   "                int, void*, size_t, void*) = mli_decode_scan_paged_alibi;\n"
                   "    int (*lean)(void* const*, const int*, const void*, const void*, const void*, const int*, float*, float*,\n"
                   "                int, int, int, int, int, int, int, int, const float*, int, void*, size_t, void*)\n"
                   "        = mli_paged_attention_lean_alibi;\n"
                   "    int (*slopes)(int, float*) = mli_alibi_slopes;\n"
                   "    int (*set)(mli_engine*, const float*, int) = mli_engine_set_alibi;\n"
                   "    (void)scan; (void)lean; (void)slopes; (void)set;\n"
                   "    return mli_abi_version() == 4 ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
