"""The multi-head entry points at the drop-in boundary, without a GPU: the symbols exist and are bound, the workspace
query is consistent with the single-head one, and unsupported shapes are refused before anything touches a device
(null device pointers: validation precedes every GPU call)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
SYMBOLS = ("mli_attention_heads_workspace_bytes", "mli_decode_scan_paged_heads", "mli_paged_attention_lean_heads",
           "mli_engine_set_heads")


def test_symbols_are_exported_and_bound(mli):
    from min_llm_inference_amd import _lib
    for name in SYMBOLS:
        assert hasattr(mli, name), name
        assert name in _lib.SIGNATURES or name in _lib.ENGINE_SIGNATURES, name
    assert mli.mli_abi_version() == 4          # no existing signature changed


def test_workspace_covers_the_single_head_workspace(mli):
    for B in (1, 8, 40, 1024, 16384):
        for S in (16, 64, 256, 4096):
            for D, heads in ((64, (2,)), (192, (3, 6)), (256, (2, 4, 8)), (512, (2, 4, 8, 16)), (1024, (4, 8, 16, 32))):
                plain = mli.mli_attention_workspace_bytes(B, S, D)
                assert mli.mli_attention_heads_workspace_bytes(B, S, D, 1) == plain
                for H in heads:
                    assert mli.mli_attention_heads_workspace_bytes(B, S, D, H) >= plain > 65536, (B, S, D, H)
    # unsupported combinations: 0
    assert mli.mli_attention_heads_workspace_bytes(8, 64, 128, 3) == 0        # emb_dim % H
    assert mli.mli_attention_heads_workspace_bytes(8, 64, 128, 8) == 0        # head_dim 16
    assert mli.mli_attention_heads_workspace_bytes(8, 64, 1024, 2) == 0       # head_dim 512
    assert mli.mli_attention_heads_workspace_bytes(8, 72, 128, 2) == 0        # n_sequence % 16
    assert mli.mli_attention_heads_workspace_bytes(16385, 64, 128, 2) == 0    # beyond the arrival counters
    assert mli.mli_attention_heads_workspace_bytes(8, 64, 2048, 8) == 0       # wider than two lane loads
    # (items x heads) statistics beyond what the merging workgroup can stage, even at 1024 tokens per item
    assert mli.mli_attention_heads_workspace_bytes(2, 131072, 1024, 32) > 0
    assert mli.mli_attention_heads_workspace_bytes(2, 131088, 1024, 32) == 0


BAD = [("emb_dim % H", 8, 64, 128, 3, F32), ("head_dim 16", 8, 64, 128, 8, F32), ("head_dim 512", 8, 64, 1024, 2, BF16),
       ("fp8 pages", 8, 64, 512, 8, FP8), ("fp32 emb_dim 1024", 8, 64, 1024, 8, F32), ("bf16 emb_dim 2048", 8, 64, 2048, 8, BF16),
       ("n_sequence % 16", 8, 72, 128, 2, F32), ("n_batch > 16384", 16385, 64, 128, 2, F32), ("n_heads 0", 8, 64, 128, 0, F32),
       ("too many items x heads", 2, 131088, 1024, 32, BF16)]


@pytest.mark.parametrize("what,B,S,D,H,elem", BAD, ids=[b[0] for b in BAD])
def test_unsupported_shapes_are_refused_before_any_launch(mli, what, B, S, D, H, elem):
    assert mli.mli_decode_scan_paged_heads(None, None, None, None, B, S, D, H, elem, None, 0, None) == BAD_ARG
    assert mli.mli_paged_attention_lean_heads(None, None, None, None, None, None, None, None, B, S, D, 0, H, elem, None, 0,
                                              None) == BAD_ARG


def test_a_missing_workspace_on_a_multi_item_shape_is_a_workspace_error(mli):
    """B 8, S 1024: several items per row, so the scans need the workspace body; validation precedes every launch.  The
    multi-head scan says MLI_ERR_WORKSPACE, the plain lean scan "not applicable", which its entry point reports as a bad
    argument."""
    assert mli.mli_decode_scan_paged_heads(None, None, None, None, 8, 1024, 128, 2, F32, None, 0, None) == WORKSPACE
    assert mli.mli_decode_scan_paged(None, None, None, None, None, 8, 1024, 128, F32, 7, None, 0, None) == BAD_ARG


def test_headers_still_compile_as_c99_and_cxx17(tmp_path):
    src = tmp_path / "heads.c"
    src.write_text('#include "mli_kernels.h"\n#include "mli_engine.h"\n'
                   "int main(void) {\n"
                   "    size_t n = mli_attention_heads_workspace_bytes(8, 64, 128, 4);\n"
                   "    int (*scan)(const float*, const void* const*, const int*, float*, int, int, int, int, int, void*, size_t,\n"
                   "                void*) = mli_decode_scan_paged_heads;\n"
                   "    int (*set)(mli_engine*, int) = mli_engine_set_heads;\n"
                   "    (void)scan; (void)set;\n"
                   "    return n > 0 ? 0 : 1;\n}\n")
    inc = os.path.join(ROOT, "include")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
