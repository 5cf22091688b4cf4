"""The sliding-window entry points at the drop-in boundary, without a GPU: the symbols exist and are bound, the ABI version
is unchanged, and a bad window, a bad head count and every unsupported shape are refused before anything touches a device
(null device pointers: validation precedes every GPU call)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
SYMBOLS = ("mli_decode_scan_paged_window", "mli_paged_attention_lean_window", "mli_engine_set_window")


def _scan(mli, B, S, D, H, W, elem):
    return mli.mli_decode_scan_paged_window(None, None, None, None, B, S, D, H, W, elem, None, 0, None)


def _lean(mli, B, S, D, H, W, elem):
    return mli.mli_paged_attention_lean_window(None, None, None, None, None, None, None, None, B, S, D, 0, H, W, elem, None, 0,
                                               None)


def test_symbols_are_exported_and_bound(mli):
    from min_llm_inference_amd import _lib
    for name in SYMBOLS:
        assert hasattr(mli, name), name
        assert name in _lib.SIGNATURES or name in _lib.ENGINE_SIGNATURES, name
    assert mli.mli_abi_version() == 4          # no existing signature changed


@pytest.mark.parametrize("H,elem", [(1, F32), (1, BF16), (1, FP8), (2, F32), (4, BF16)])
@pytest.mark.parametrize("W", [0, -1])
def test_a_window_below_one_is_refused(mli, W, H, elem):
    for S in (64, 16):          # also where the window would otherwise count as "no window"
        assert _scan(mli, 8, S, 128, H, W, elem) == BAD_ARG
        assert _lean(mli, 8, S, 128, H, W, elem) == BAD_ARG


@pytest.mark.parametrize("W", [1, 12, 63, 64, 1000])
def test_no_heads_is_refused(mli, W):
    for elem in (F32, BF16, FP8):
        assert _scan(mli, 8, 64, 128, 0, W, elem) == BAD_ARG
        assert _lean(mli, 8, 64, 128, 0, W, elem) == BAD_ARG
        assert _scan(mli, 8, 64, 128, -2, W, elem) == BAD_ARG


# every shape heads_shape_supported refuses with n_heads > 1 (tests/test_heads_abi.py)
BAD_HEADS = [("emb_dim % H", 8, 64, 128, 3, F32), ("head_dim 16", 8, 64, 128, 8, F32), ("head_dim 512", 8, 64, 1024, 2, BF16),
             ("fp8 pages", 8, 64, 512, 8, FP8), ("fp32 emb_dim 1024", 8, 64, 1024, 8, F32),
             ("bf16 emb_dim 2048", 8, 64, 2048, 8, BF16), ("n_sequence % 16", 8, 72, 128, 2, F32),
             ("n_batch > 16384", 16385, 64, 128, 2, F32), ("too many items x heads", 2, 131088, 1024, 32, BF16)]
# one head: what the lean chunked scan does not take
BAD_PLAIN = [("n_sequence % 16", 8, 72, 128, 1, F32), ("n_sequence % 16 bf16", 8, 40, 128, 1, BF16),
             ("n_sequence % 16 fp8", 8, 72, 128, 1, FP8), ("n_batch 16385", 16385, 64, 128, 1, F32),
             ("n_batch 16385 bf16", 16385, 64, 128, 1, BF16), ("n_batch 0", 0, 64, 128, 1, F32),
             ("fp32 emb_dim 2052", 8, 64, 2052, 1, F32), ("bf16 emb_dim 4104", 8, 64, 4104, 1, BF16),
             ("bf16 emb_dim % 8", 8, 64, 132, 1, BF16), ("fp8 emb_dim % 16", 8, 64, 136, 1, FP8),
             ("fp8 emb_dim 2064", 8, 64, 2064, 1, FP8), ("element type 3", 8, 64, 128, 1, 3)]


@pytest.mark.parametrize("what,B,S,D,H,elem", BAD_HEADS + BAD_PLAIN, ids=[b[0] for b in BAD_HEADS + BAD_PLAIN])
def test_unsupported_shapes_are_refused_before_any_launch(mli, what, B, S, D, H, elem):
    for W in (1, 12, S - 1):
        assert _scan(mli, B, S, D, H, W, elem) == BAD_ARG, W
        assert _lean(mli, B, S, D, H, W, elem) == BAD_ARG, W


@pytest.mark.parametrize("H", [1, 2])
def test_a_missing_workspace_on_a_multi_item_shape_is_a_workspace_error(mli, H):
    """B 8, S 1024, W 256: several items per row, so the scan needs the workspace body; validation precedes every launch."""
    assert _scan(mli, 8, 1024, 128, H, 256, F32) == WORKSPACE


def test_headers_still_compile_as_c99_and_cxx17(tmp_path):
    src = tmp_path / "window.c"
    src.write_text('#include "mli_kernels.h"\n#include "mli_engine.h"\n'
                   "int main(void) {\n"
                   "    int (*scan)(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, void*,\n"
                   "                size_t, void*) = mli_decode_scan_paged_window;\n"
                   "    int (*lean)(void* const*, const int*, const void*, const void*, const void*, const int*, float*, float*,\n"
                   "                int, int, int, int, int, int, int, void*, size_t, void*) = mli_paged_attention_lean_window;\n"
                   "    int (*set)(mli_engine*, int) = mli_engine_set_window;\n"
                   "    (void)scan; (void)lean; (void)set;\n"
                   "    return mli_abi_version() == 4 ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
