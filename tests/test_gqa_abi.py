"""The grouped-query entry points at the drop-in boundary, without a GPU: the symbols exist and are bound, the ABI version is
unchanged, bad head counts, fp8 pages and every unsupported shape are refused before anything touches a device (null device
pointers: validation precedes every GPU call), a multi-item shape without a workspace is a workspace error, n_kv_heads ==
n_heads answers what the entry point with sinks answers, the headers compile as C99 and C++17, and the engine setter refuses
a null handle."""
import os
import shutil
import subprocess

import pytest

from test_window_abi import BAD_HEADS, BAD_PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
SYMBOLS = ("mli_decode_scan_paged_gqa", "mli_paged_attention_lean_gqa", "mli_engine_set_kv_heads")
FORMS = ((0, 0), (-3, 0), (12, 0), (12, 4), (0, 4), (1000000, 4))     # (window, n_sink)


def _scan(mli, B, S, D, H, Hkv, W, K, elem):
    return mli.mli_decode_scan_paged_gqa(None, None, None, None, B, S, D, H, Hkv, W, K, elem, None, 0, None)


def _lean(mli, B, S, D, H, Hkv, W, K, elem):
    return mli.mli_paged_attention_lean_gqa(None, None, None, None, None, None, None, None, B, S, D, 0, H, Hkv, W, K, elem, None,
                                            0, None)


def _sinks(mli, B, S, D, H, W, K, elem):
    return mli.mli_decode_scan_paged_sinks(None, None, None, None, B, S, D, H, W if W >= 1 else S, K, elem, None, 0, None)


def test_symbols_are_exported_and_bound(mli):
    from min_llm_inference_amd import _lib
    for name in SYMBOLS:
        assert hasattr(mli, name), name
        assert name in _lib.SIGNATURES or name in _lib.ENGINE_SIGNATURES, name
    assert len(_lib.SIGNATURES["mli_decode_scan_paged_gqa"]) == 15 and len(_lib.SIGNATURES["mli_paged_attention_lean_gqa"]) == 20
    assert mli.mli_abi_version() == 4          # no existing signature changed


@pytest.mark.parametrize("H,Hkv", [(8, 3), (8, 5), (8, 0), (8, -1), (8, 16), (8, 9), (6, 4), (2, 3), (1, 2), (1, 0), (0, 1), (0, 0),
                                   (-2, 1), (3, 2)])
def test_bad_head_counts_are_refused(mli, H, Hkv):
    for elem in (F32, BF16, FP8):
        for S in (64, 1024):
            for W, K in FORMS:
                assert _scan(mli, 8, S, 192 if H in (3, 6) else 256, H, Hkv, W, K, elem) == BAD_ARG, (S, W, K, elem)
                assert _lean(mli, 8, S, 192 if H in (3, 6) else 256, H, Hkv, W, K, elem) == BAD_ARG, (S, W, K, elem)


@pytest.mark.parametrize("H,Hkv", [(8, 4), (8, 1), (8, 8), (2, 1), (1, 1)])
def test_fp8_pages_and_negative_sinks_are_refused(mli, H, Hkv):
    for W, K in FORMS:
        assert _scan(mli, 8, 64, 256, H, Hkv, W, K, FP8) == BAD_ARG        # fp8 pages have no heads, grouped or not
        assert _lean(mli, 8, 64, 256, H, Hkv, W, K, FP8) == BAD_ARG
        assert _scan(mli, 8, 64, 256, H, Hkv, W, K, 3) == BAD_ARG
    for elem in (F32, BF16):
        for W in (0, 12, 64):
            assert _scan(mli, 8, 64, 256, H, Hkv, W, -1, elem) == BAD_ARG
            assert _lean(mli, 8, 64, 256, H, Hkv, W, -1, elem) == BAD_ARG


@pytest.mark.parametrize("what,B,S,D,H,elem", BAD_HEADS + BAD_PLAIN, ids=[b[0] for b in BAD_HEADS + BAD_PLAIN])
def test_unsupported_shapes_are_refused_before_any_launch(mli, what, B, S, D, H, elem):
    """everything the heads / window entry points refuse, grouped (every divisor of H) and through the n_kv_heads == n_heads
    hand-off; plain, windowed and with sinks.  (One head without a window is the plain single-head scan, whose answers
    tests/test_error_paths.py holds: not repeated here.)"""
    for Hkv in [d for d in range(1, H + 1) if H % d == 0]:
        for W, K in ((0, 0), (12, 0), (12, 4), (S - 2, 1), (S, 0)):
            if H == 1 and (W <= 0 or W >= S) and elem in (F32, BF16):
                continue
            assert _scan(mli, B, S, D, H, Hkv, W, K, elem) == BAD_ARG, (Hkv, W, K)
            assert _lean(mli, B, S, D, H, Hkv, W, K, elem) == BAD_ARG, (Hkv, W, K)


@pytest.mark.parametrize("H,Hkv", [(2, 1), (4, 2), (4, 1)])
def test_a_missing_workspace_on_a_multi_item_shape_is_a_workspace_error(mli, H, Hkv):
    """B 8, S 1024: several items per row, plain, windowed and with sinks -- the scan needs the workspace body and says so
    before any launch; the workspace query is the multi-head one, unchanged."""
    for W, K in ((0, 0), (256, 0), (256, 4), (2000, 4), (256, 768)):
        for elem in (F32, BF16):
            assert _scan(mli, 8, 1024, 128, H, Hkv, W, K, elem) == WORKSPACE, (W, K, elem)
    # 64 KiB of arrival counters | statistics | the worst case of ceil(S / 64) partial rows per row
    assert mli.mli_attention_heads_workspace_bytes(8, 1024, 128, H) >= 65536 + 8 * 16 * H * 8 + 8 * 16 * 128 * 4
    assert not hasattr(mli, "mli_attention_gqa_workspace_bytes")


def test_every_group_size_passes_validation(mli):
    """g = 3 and the other group sizes are accepted: with B 8, S 1024 the refusal is the workspace's, not the arguments'"""
    for D, H, Hkv in ((192, 3, 1), (192, 6, 2), (192, 6, 3), (256, 8, 1), (512, 16, 4), (512, 8, 2)):
        assert _scan(mli, 8, 1024, D, H, Hkv, 0, 0, BF16) == WORKSPACE, (D, H, Hkv)


@pytest.mark.parametrize("H", [1, 2, 4])
def test_equal_head_counts_are_the_entry_point_with_sinks(mli, H):
    """n_kv_heads == n_heads is handed on before anything else: the status is mli_decode_scan_paged_sinks's (window <= 0: a
    window of n_sequence there), n_heads = 1 included"""
    for elem in (F32, BF16):
        for W, K in ((0, 0), (-1, 0), (256, 0), (256, 4), (256, 768), (4000, 4), (0, 4)):
            assert _scan(mli, 8, 1024, 128, H, H, W, K, elem) == _sinks(mli, 8, 1024, 128, H, W, K, elem), (W, K, elem)


def test_the_engine_setter_refuses_a_null_handle(mli):
    for n in (1, 2, 0):
        assert mli.mli_engine_set_kv_heads(None, n) == -1
        assert b"null argument" in mli.mli_engine_last_error()


def test_headers_still_compile_as_c99_and_cxx17(tmp_path):
    src = tmp_path / "gqa.c"
    src.write_text('#include "mli_kernels.h"\n#include "mli_engine.h"\n'
                   "int main(void) {\n"
                   "    int (*scan)(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, int, int, void*,\n"
                   "                size_t, void*) = mli_decode_scan_paged_gqa;\n"
                   "    int (*lean)(void* const*, const int*, const void*, const void*, const void*, const int*, float*, float*,\n"
                   "                int, int, int, int, int, int, int, int, int, void*, size_t, void*) = mli_paged_attention_lean_gqa;\n"
                   "    int (*set)(mli_engine*, int) = mli_engine_set_kv_heads;\n"
                   "    (void)scan; (void)lean; (void)set;\n"
                   "    return mli_abi_version() == 4 ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
