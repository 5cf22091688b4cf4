"""The rotary-embedding entry points at the drop-in boundary, without a GPU: the symbols exist and are bound with their arity,
the ABI version is unchanged, mli_rope_table refuses what it must, and every *_rope call refuses a null table, bad head counts,
an odd head_dim, and everything its un-rotated entry point refuses -- before anything touches a device (null device pointers
and launch counters that stay at zero: an accepted call could not be mistaken for a refused one, it would not come back with
MLI_ERR_BAD_ARG).  The refusal tables of the _alibi and _gqa entry points hold through mli_paged_attention_lean_rope.  The
one accepted call made here is a fill of zero new rows, which returns 0 without a launch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_window_abi import BAD_HEADS, BAD_PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, F32, BF16, FP8 = -22, 0, 1, 2
SYMBOLS = {"mli_rope_table": 4, "mli_get_latest_k_q_v_paged_rope": 13, "mli_fill_new_k_v_cache_paged_rope": 13,
           "mli_paged_prefill_rope": 18, "mli_paged_attention_lean_rope": 22}
FAMILIES = (b"gemm_f32_rope", b"gemm_bf16_rope", b"gemm_f32_rows64", b"gemm_f32_rows64_split", b"gemm_f32_rows128", b"gemm_f32_panel",
            b"gemm_bf16_rows64", b"gemm_bf16_deep", b"gemm_bf16_rows128", b"gemm_bf16_dma", b"gemm_bf16_fill", b"gemm_bf16_widened",
            b"scan_heads_window", b"scan_heads_alibi", b"scan_chunked", b"prefill_fused", b"prefill_two_launch")
TABLE = ctypes.c_void_p(256)       # non-null addresses nobody follows: every call here ends before a launch
SLOPES = ctypes.c_void_p(512)
PTR = ctypes.c_void_p(1024)


def _latest(mli, B, S, D, H, elem, table=TABLE):
    return mli.mli_get_latest_k_q_v_paged_rope(None, None, None, None, None, None, B, S, D, H, table, elem, None)


def _fill(mli, B, S, D, H, elem, table=TABLE, n_new=0):
    return mli.mli_fill_new_k_v_cache_paged_rope(None, None, None, None, None, B, S, D, n_new, H, table, elem, None)


def _prefill(mli, B, S, D, H, elem, table=TABLE, n_new=0, W=0, K=0, emb=PTR):
    return mli.mli_paged_prefill_rope(emb, emb, emb, None, None, None, None, None, B, S, D, n_new, W, K, H, table, elem, None)


def _lean(mli, B, S, D, H, Hkv, W, K, elem, slopes=None, table=TABLE):
    return mli.mli_paged_attention_lean_rope(None, None, None, None, None, None, None, None, B, S, D, 0, H, Hkv, W, K, slopes, table,
                                             elem, None, 0, None)


@pytest.fixture(autouse=True)
def nothing_is_launched(mli):
    assert mli.mli_launch_counts_reset() == 0
    yield
    n = ctypes.c_ulonglong(99)
    for family in FAMILIES:
        assert mli.mli_launch_count(family, ctypes.byref(n)) == 0 and n.value == 0, family


def test_symbols_are_exported_and_bound(mli):
    import inspect
    from min_llm_inference_amd import _lib, ops
    for name, arity in SYMBOLS.items():
        assert hasattr(mli, name), name
        assert len(_lib.SIGNATURES[name]) == arity, name
    assert mli.mli_abi_version() == 4          # no existing signature changed
    assert callable(ops.rope_table) and callable(ops.fill_new_k_v_cache_paged_rope)
    for fn in (ops.get_latest_k_q_v_paged_lean, ops.paged_prefill, ops.paged_attention_lean):
        assert "rope" in inspect.signature(fn).parameters, fn.__name__
    for fn in (ops.get_latest_k_q_v_paged_lean, ops.paged_prefill):
        assert "n_heads" in inspect.signature(fn).parameters, fn.__name__
    n = ctypes.c_ulonglong(99)
    for family in (b"gemm_f32_rope", b"gemm_bf16_rope"):
        assert mli.mli_launch_count(family, ctypes.byref(n)) == 0 and n.value == 0


def test_rope_table_refusals(mli):
    out = np.zeros(64 * 32, np.float32)
    p = out.ctypes.data_as(ctypes.c_void_p)
    assert mli.mli_rope_table(64, 32, 10000.0, p) == 0
    for S, hd, theta, ptr in ((64, 32, 10000.0, None), (0, 32, 10000.0, p), (-1, 32, 10000.0, p), (64, 31, 10000.0, p),
                              (64, 0, 10000.0, p), (64, 1, 10000.0, p), (64, -2, 10000.0, p), (64, 32, 0.0, p), (64, 32, -1.0, p),
                              (64, 32, float("inf"), p), (64, 32, float("nan"), p)):
        assert mli.mli_rope_table(S, hd, theta, ptr) == BAD_ARG, (S, hd, theta)


@pytest.mark.parametrize("elem,D", [(F32, 128), (BF16, 128), (FP8, 128)])
def test_rope_arguments_are_refused(mli, elem, D):
    ok = dict(B=8, S=64, D=D, H=4, elem=elem)
    assert _fill(mli, **ok) == 0 and _prefill(mli, **ok) == 0      # zero new rows: accepted, nothing launched
    assert _prefill(mli, W=32, K=4, **ok) == 0
    for call in (_latest, _fill, _prefill):
        assert call(mli, table=None, **ok) == BAD_ARG, call.__name__
        for H in (0, -1, 3, 5, 7, 128, 256):     # n_heads < 1, emb_dim % n_heads, an odd head_dim (128 heads of 1)
            assert call(mli, **dict(ok, H=H)) == BAD_ARG, (call.__name__, H)
        assert call(mli, **dict(ok, elem=3)) == BAD_ARG and call(mli, **dict(ok, elem=-1)) == BAD_ARG
        # what the un-rotated call refuses (a fill of zero new rows returns 0 before it looks at anything else, as there)
        new = {} if call is _latest else {"n_new": 2}
        assert call(mli, **dict(ok, B=0, **new)) == BAD_ARG and call(mli, **dict(ok, S=72, **new)) == BAD_ARG
        assert call(mli, **dict(ok, D={F32: 66, BF16: 132, FP8: 136}[elem], H=1, **new)) == BAD_ARG
    assert _lean(mli, 8, 64, D, 4, 4, 0, 0, elem, table=None) == BAD_ARG
    assert _fill(mli, n_new=-1, **ok) == BAD_ARG and _prefill(mli, n_new=-1, **ok) == BAD_ARG
    assert _prefill(mli, emb=None, **ok) == BAD_ARG
    assert _prefill(mli, W=-1, **ok) == BAD_ARG and _prefill(mli, W=32, K=-1, **ok) == BAD_ARG


def test_an_fp32_emb_dim_of_66_is_refused_as_without_the_table(mli):
    """emb_dim 66 with one head has an even head_dim, but no paged fp32 entry point takes an emb_dim that is no multiple of 4:
    the scalar-load form of the kernel runs for weights that are not 16-byte aligned (tests/test_rope_gemm_gpu.py)."""
    assert mli.mli_get_latest_k_q_v_paged_lean(None, None, None, None, None, None, 8, 64, 66, F32, None) == BAD_ARG
    assert _latest(mli, 8, 64, 66, 1, F32) == BAD_ARG
    assert mli.mli_fill_new_k_v_cache_paged(None, None, None, None, None, 8, 64, 66, 2, None) == BAD_ARG
    assert _fill(mli, 8, 64, 66, 1, F32, n_new=2) == BAD_ARG


@pytest.mark.parametrize("slopes", [None, SLOPES], ids=["gqa", "alibi"])
def test_lean_rope_refuses_bad_head_counts(mli, slopes):
    for H, Hkv in [(8, 3), (8, 5), (8, 0), (8, -1), (8, 16), (8, 9), (6, 4), (2, 3), (1, 2), (1, 0), (0, 1), (0, 0), (-2, 1), (3, 2)]:
        for elem in (F32, BF16, FP8):
            for S in (64, 1024):
                for W, K in ((0, 0), (-3, 0), (40, 0), (40, 4), (0, 4), (1000000, 4)):
                    assert _lean(mli, 8, S, 192 if H in (3, 6) else 256, H, Hkv, W, K, elem, slopes) == BAD_ARG, (H, Hkv, S, W, K, elem)


def test_lean_rope_keeps_the_alibi_rules(mli):
    for elem in (F32, BF16, FP8):
        for W, K in ((0, 0), (40, 0), (40, 4)):
            assert _lean(mli, 8, 64, 128, 1, 1, W, K, elem, SLOPES) == BAD_ARG          # one head has no bias
    for H, Hkv in [(8, 4), (8, 1), (8, 8), (2, 1)]:
        for W, K in ((0, 0), (40, 0), (40, 4)):
            assert _lean(mli, 8, 64, 256, H, Hkv, W, K, FP8, SLOPES) == BAD_ARG         # fp8 pages
            assert _lean(mli, 8, 64, 256, H, Hkv, W, K, FP8, None) == BAD_ARG           # ... and several heads without a bias
        for elem in (F32, BF16):
            assert _lean(mli, 8, 64, 256, H, Hkv, 40, -1, elem, SLOPES) == BAD_ARG
            assert _lean(mli, 8, 64, 256, H, Hkv, 40, -1, elem, None) == BAD_ARG


@pytest.mark.parametrize("what,B,S,D,H,elem", BAD_HEADS + BAD_PLAIN, ids=[b[0] for b in BAD_HEADS + BAD_PLAIN])
def test_lean_rope_refuses_unsupported_shapes_before_any_launch(mli, what, B, S, D, H, elem):
    """the tables of tests/test_gqa_abi.py and tests/test_alibi_abi.py through _lean_rope, with every divisor of H as n_kv_heads.
    (One head without a window is the plain single-head scan, which judges its shape itself: not asked here, as there.)"""
    if D % H != 0 or (D // H) % 2 != 0:
        assert _lean(mli, B, S, D, H, H, 0, 0, elem) == BAD_ARG
    for Hkv in [d for d in range(1, H + 1) if H % d == 0]:
        for W, K in ((0, 0), (12, 0), (12, 4), (S - 2, 1), (S, 0)):
            assert _lean(mli, B, S, D, H, Hkv, W, K, elem, SLOPES) == BAD_ARG, (Hkv, W, K)
            if H == 1 and (W <= 0 or W >= S):
                continue
            assert _lean(mli, B, S, D, H, Hkv, W, K, elem, None) == BAD_ARG, (Hkv, W, K)


def test_headers_still_compile_as_c99_and_cxx17(tmp_path):
    src = tmp_path / "rope.c"
    src.write_text('#include "mli_kernels.h"\n#include "mli_engine.h"\n'
                   "int main(void) {\n"
                   "    int (*table)(int, int, double, float*) = mli_rope_table;\n"
                   "    int (*latest)(void* const*, const int*, const void*, const void*, const void*, float*, int, int, int, int,\n"
                   "                  const float*, int, void*) = mli_get_latest_k_q_v_paged_rope;\n"
                   "    int (*fill)(void* const*, const int*, const int*, const void*, const void*, int, int, int, int, int,\n"
                   "                const float*, int, void*) = mli_fill_new_k_v_cache_paged_rope;\n"
                   "    int (*prefill)(const float*, const float*, const int*, void* const*, const int*, const int*, const void*,\n"
                   "                   const void*, int, int, int, int, int, int, int, const float*, int, void*) = mli_paged_prefill_rope;\n"
                   "    int (*lean)(void* const*, const int*, const void*, const void*, const void*, const int*, float*, float*,\n"
                   "                int, int, int, int, int, int, int, int, const float*, const float*, int, void*, size_t, void*)\n"
                   "        = mli_paged_attention_lean_rope;\n"
                   "    (void)table; (void)latest; (void)fill; (void)prefill; (void)lean;\n"
                   "    return mli_abi_version() == 4 ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
