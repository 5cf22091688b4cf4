"""The attention-sink entry points at the drop-in boundary, without a GPU: the symbols exist and are bound, the ABI version
is unchanged, a bad sink count, window or head count and every unsupported shape are refused before anything touches a
device (null device pointers: validation precedes every GPU call), the hand-offs (K = 0, K + W >= n_sequence) are not
refused, and the workspace is the un-windowed one."""
import os
import shutil
import subprocess

import pytest

from test_window_abi import BAD_HEADS, BAD_PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
SYMBOLS = ("mli_decode_scan_paged_sinks", "mli_paged_attention_lean_sinks", "mli_engine_set_sinks")


def _scan(mli, B, S, D, H, W, K, elem):
    return mli.mli_decode_scan_paged_sinks(None, None, None, None, B, S, D, H, W, K, elem, None, 0, None)


def _lean(mli, B, S, D, H, W, K, elem):
    return mli.mli_paged_attention_lean_sinks(None, None, None, None, None, None, None, None, B, S, D, 0, H, W, K, elem, None,
                                              0, None)


def test_symbols_are_exported_and_bound(mli):
    from min_llm_inference_amd import _lib
    for name in SYMBOLS:
        assert hasattr(mli, name), name
        assert name in _lib.SIGNATURES or name in _lib.ENGINE_SIGNATURES, name
    assert mli.mli_abi_version() == 4          # no existing signature changed


@pytest.mark.parametrize("H,elem", [(1, F32), (1, BF16), (1, FP8), (2, F32), (4, BF16)])
def test_bad_counts_are_refused(mli, H, elem):
    for S in (64, 16):          # also where the call would otherwise be handed to the un-windowed entry points
        for W, K in ((12, -1), (12, -100), (0, 4), (-1, 4), (0, 0), (S, -1), (0, S)):
            assert _scan(mli, 8, S, 128, H, W, K, elem) == BAD_ARG, (S, W, K)
            assert _lean(mli, 8, S, 128, H, W, K, elem) == BAD_ARG, (S, W, K)


@pytest.mark.parametrize("W,K", [(1, 1), (12, 4), (12, 0), (12, 52), (63, 4), (64, 4), (1000, 0)])
def test_no_heads_is_refused(mli, W, K):
    for elem in (F32, BF16, FP8):
        assert _scan(mli, 8, 64, 128, 0, W, K, elem) == BAD_ARG
        assert _lean(mli, 8, 64, 128, 0, W, K, elem) == BAD_ARG
        assert _scan(mli, 8, 64, 128, -2, W, K, elem) == BAD_ARG


@pytest.mark.parametrize("what,B,S,D,H,elem", BAD_HEADS + BAD_PLAIN, ids=[b[0] for b in BAD_HEADS + BAD_PLAIN])
def test_unsupported_shapes_are_refused_before_any_launch(mli, what, B, S, D, H, elem):
    """exactly what window_shape_supported refuses, with sinks (K >= 1, K + W < S) and through the K = 0 hand-off"""
    for W, K in ((1, 1), (12, 4), (12, 0), (S - 2, 1), (5, 17)):
        assert _scan(mli, B, S, D, H, W, K, elem) == BAD_ARG, (W, K)
        assert _lean(mli, B, S, D, H, W, K, elem) == BAD_ARG, (W, K)


@pytest.mark.parametrize("H", [1, 2])
def test_the_workspace_rule(mli, H):
    """B 8, S 1024, W 256, K 4: several items per row, so the scan needs the workspace body and says so before any launch
    (validation precedes it).  That what it needs is within the un-windowed workspace of the same (n_batch, n_sequence,
    emb_dim, n_heads) is NOT shown here -- without a device no buffer can be handed in, and the last line only holds the
    size queries to the layout's worst case; tests/cpp/sink_plan_test.cpp holds the sinks' plan to that worst case and
    tests/test_sinks_scan_gpu.py runs a scan with sinks in a buffer of exactly the plain size."""
    assert _scan(mli, 8, 1024, 128, H, 256, 4, F32) == WORKSPACE
    assert _scan(mli, 8, 1024, 128, H, 256, 0, F32) == WORKSPACE        # K = 0: the windowed scan
    assert _lean_needs_no_more(mli, H)


def _lean_needs_no_more(mli, H):
    plain = mli.mli_attention_workspace_bytes(8, 1024, 128) if H == 1 else mli.mli_attention_heads_workspace_bytes(8, 1024, 128, H)
    # 64 KiB of arrival counters | statistics | the worst case of ceil(S / 64) partial rows per row
    return plain >= 65536 + 8 * 16 * H * 8 + 8 * 16 * 128 * 4


def test_hand_offs_are_not_refused(mli):
    """K + W >= n_sequence, W >= n_sequence and K = 0 go to the existing entry points before the sinks' own shape check:
    the status is theirs.  With null pointers and no workspace the multi-head and the windowed scan answer a multi-item
    shape with a workspace error, not a bad argument; the plain one-head scan answers what it answers when called itself."""
    for W, K in ((256, 768), (256, 4000), (1024, 4), (5000, 0), (1023, 1)):
        assert _scan(mli, 8, 1024, 128, 2, W, K, F32) == WORKSPACE, (W, K)
        plain = mli.mli_decode_scan_paged(None, None, None, None, None, 8, 1024, 128, F32, 7, None, 0, None)
        assert _scan(mli, 8, 1024, 128, 1, W, K, F32) == plain, (W, K)
    for W in (256, 1023):          # (several items per row: nothing is launched)
        assert _scan(mli, 8, 1024, 128, 1, W, 0, BF16) == WORKSPACE, W
    # a hand-off is the other entry point with its own refusals: fp8 pages have no heads there either
    assert _scan(mli, 8, 1024, 128, 2, 1024, 4, FP8) == BAD_ARG
    assert _scan(mli, 8, 1024, 128, 2, 256, 768, FP8) == BAD_ARG


def test_headers_still_compile_as_c99_and_cxx17(tmp_path):
    src = tmp_path / "sinks.c"
    src.write_text('#include "mli_kernels.h"\n#include "mli_engine.h"\n'
                   "int main(void) {\n"
                   "    int (*scan)(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, int, void*,\n"
                   "                size_t, void*) = mli_decode_scan_paged_sinks;\n"
                   "    int (*lean)(void* const*, const int*, const void*, const void*, const void*, const int*, float*, float*,\n"
                   "                int, int, int, int, int, int, int, int, void*, size_t, void*) = mli_paged_attention_lean_sinks;\n"
                   "    int (*set)(mli_engine*, int) = mli_engine_set_sinks;\n"
                   "    (void)scan; (void)lean; (void)set;\n"
                   "    return mli_abi_version() == 4 ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
