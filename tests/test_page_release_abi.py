"""Early page release at the drop-in boundary, without a GPU: the new symbols exist and are bound, the ABI version is
unchanged, mli_paged_prefill_window refuses a negative window or sink count and every shape mli_paged_prefill refuses before
anything touches a device (null or never-followed pointers: validation precedes every GPU call), and the windows that leave
no row a dead page answer what mli_paged_prefill answers."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, F32, BF16, FP8 = -22, 0, 1, 2
SYMBOLS = ("mli_paged_prefill_window", "mli_engine_set_page_release", "mli_engine_get_page_stats")
FAKE = ctypes.c_void_p(4096)      # a non-null pointer no refused call follows


def _plain(mli, B, S, D, n_new, elem, ptr=None):
    return mli.mli_paged_prefill(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, S, D, n_new, elem, None)


def _window(mli, B, S, D, n_new, W, K, elem, ptr=None):
    return mli.mli_paged_prefill_window(ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, S, D, n_new, W, K, elem, None)


def test_symbols_are_exported_and_bound(mli):
    from min_llm_inference_amd import _lib, engine, ops
    for name in SYMBOLS:
        assert hasattr(mli, name), name
        assert name in _lib.SIGNATURES or name in _lib.ENGINE_SIGNATURES, name
    assert mli.mli_abi_version() == 4          # additions only
    assert ctypes.sizeof(_lib.EnginePageStats) == 32
    assert hasattr(engine.Engine, "set_page_release") and hasattr(engine.Engine, "page_stats")
    assert ops.paged_prefill.__code__.co_varnames[:12][-2:] == ("window", "sinks")


@pytest.mark.parametrize("elem", [F32, BF16, FP8])
def test_negative_counts_are_refused(mli, elem):
    for S in (256, 16):
        for W, K in ((-1, 0), (-5, 4), (12, -1), (0, -1), (S, -1), (-1, S), (-1, -1)):
            assert _window(mli, 8, S, 128, 2, W, K, elem) == BAD_ARG, (S, W, K)
            assert _window(mli, 8, S, 128, 2, W, K, elem, FAKE) == BAD_ARG, (S, W, K)     # before any shape is looked at
            assert _window(mli, 8, S, 128, 0, W, K, elem, FAKE) == BAD_ARG, (S, W, K)


BAD_SHAPES = [("n_sequence % 16", 8, 72, 128, 2, F32), ("emb_dim % 4", 8, 256, 130, 2, F32), ("n_batch 0", 0, 256, 128, 2, F32),
              ("n_new < 0", 8, 256, 128, -1, F32), ("bf16 emb_dim % 8", 8, 256, 132, 2, BF16), ("bf16 n_new < 0", 8, 256, 128, -3, BF16),
              ("fp8 emb_dim % 16", 8, 256, 136, 2, FP8), ("fp8 n_sequence % 16", 8, 250, 128, 2, FP8),
              ("element type 3", 8, 256, 128, 2, 3), ("element type -1", 8, 256, 128, 2, -1)]


@pytest.mark.parametrize("what,B,S,D,n_new,elem", BAD_SHAPES, ids=[b[0] for b in BAD_SHAPES])
def test_the_shapes_the_plain_prefill_refuses_are_refused(mli, what, B, S, D, n_new, elem):
    assert _plain(mli, B, S, D, n_new, elem, FAKE) == BAD_ARG
    for W, K in ((12, 0), (40, 4), (17, 16), (1, 1)):
        assert _window(mli, B, S, D, n_new, W, K, elem, FAKE) == BAD_ARG, (W, K)
    for fused in (0, 2):          # in either form
        assert mli.mli_tune(b"prefill_fused", fused) == 0
        try:
            assert _window(mli, B, S, D, n_new, 40, 4, elem, FAKE) == BAD_ARG
        finally:
            mli.mli_tune(b"prefill_fused", 1)


@pytest.mark.parametrize("elem", [F32, BF16, FP8])
def test_null_tables_are_refused_and_no_new_rows_is_a_no_op(mli, elem):
    assert _window(mli, 8, 256, 128, 2, 40, 4, elem) == BAD_ARG == _plain(mli, 8, 256, 128, 2, elem)
    for fused in (0, 1, 2):
        assert mli.mli_tune(b"prefill_fused", fused) == 0
        try:
            for D in (128, 2048):
                assert _plain(mli, 8, 256, D, 0, elem, FAKE) == 0
                assert _window(mli, 8, 256, D, 0, 40, 4, elem, FAKE) == 0
                assert _window(mli, 8, 256, D, 0, 12, 0, elem, FAKE) == 0
        finally:
            mli.mli_tune(b"prefill_fused", 1)


@pytest.mark.parametrize("W,K", [(0, 0), (0, 9), (256, 0), (1000, 4), (200, 56), (16, 240), (1, 255)])
def test_hand_offs_answer_what_the_plain_prefill_answers(mli, W, K):
    """no window, W >= n_sequence, K + W >= n_sequence: mli_paged_prefill, with its own refusals and its own no-op"""
    for elem in (F32, BF16, FP8, 3):
        for B, S, D, n_new, ptr in ((8, 256, 128, 2, None), (8, 256, 128, 0, FAKE), (8, 256, 130, 2, FAKE), (0, 256, 128, 2, FAKE),
                                    (8, 256, 128, -1, FAKE)):
            assert _window(mli, B, S, D, n_new, W, K, elem, ptr) == _plain(mli, B, S, D, n_new, elem, ptr), (elem, B, S, D, n_new)


def test_headers_still_compile_as_c99_and_cxx17(tmp_path):
    src = tmp_path / "release.c"
    src.write_text('#include "mli_kernels.h"\n#include "mli_engine.h"\n'
                   "int main(void) {\n"
                   "    int (*prefill)(const float*, const float*, const int*, void* const*, const int*, const int*, const void*,\n"
                   "                   const void*, int, int, int, int, int, int, int, void*) = mli_paged_prefill_window;\n"
                   "    int (*set)(mli_engine*, int) = mli_engine_set_page_release;\n"
                   "    int (*get)(mli_engine*, mli_engine_page_stats*) = mli_engine_get_page_stats;\n"
                   "    mli_engine_page_stats s = {0, 0, 0, 0, 0};\n"
                   "    (void)prefill; (void)set; (void)get; (void)s;\n"
                   "    return mli_abi_version() == 4 ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
