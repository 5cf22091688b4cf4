"""The sink-logit entry points at the drop-in boundary, without a GPU: the symbols exist and are bound as the header declares
them, the ABI version is unchanged, and one head, fp8 pages, bad head counts, every unsupported shape, a negative n_sink, a null
sink_logits and a null data pointer are refused before anything touches a device (the pointers given are addresses nobody
follows: validation precedes every GPU call) by both scans and both compositions; accepted shapes get past the argument check
(the refusal is then the workspace's); the two launch families are known and at zero and no refusal counts a launch in any
family; the prompt variant keeps mli_prompt_scan_tq; the headers compile as C99 and C++17 and a plain C host links and calls an
entry point; the engine setter refuses a null handle.  (An engine needs a device: the setter's other refusals, in both orders
of every refused pair, are held on a live device by tests/test_sink_logits_engine_gpu.py.)"""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from test_window_abi import BAD_HEADS, BAD_PLAIN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
SYMBOLS = ("mli_decode_scan_paged_sink_logits", "mli_paged_attention_lean_sink_logits", "mli_prompt_scan_paged_sink_logits",
           "mli_paged_prompt_logprobs_sink_logits", "mli_engine_set_sink_logits")
FAMILIES = (b"scan_heads_sink_logits", b"scan_prompt_sink_logits")
FORMS = ((0, 0), (-3, 0), (40, 0), (5, 0), (40, 4), (40, 20), (0, 4), (1000000, 4))     # (window, n_sink)
PTR = ctypes.c_void_p(256)      # a non-null address nobody follows: every call here ends before a launch


def _scan(mli, B, S, D, H, Hkv, W, K, elem, z=PTR, data=PTR):
    return mli.mli_decode_scan_paged_sink_logits(data, data, data, data, B, S, D, H, Hkv, W, K, z, elem, None, 0, None)


def _lean(mli, B, S, D, H, Hkv, W, K, elem, z=PTR, data=PTR, rope=None):
    return mli.mli_paged_attention_lean_sink_logits(data, data, data, data, data, None, data, data, B, S, D, 0, H, Hkv, W, K, z, rope,
                                                    elem, None, 0, None)


def _prompt(mli, B, S, D, H, Hkv, W, K, elem, z=PTR, data=PTR, n_seg=1):
    return mli.mli_prompt_scan_paged_sink_logits(data, data, data, data, data, data, data, n_seg, 1, 1, B, S, D, H, Hkv, W, K, z,
                                                 elem, None)


def _score(mli, B, S, D, H, Hkv, W, K, elem, z=PTR, data=PTR):
    return mli.mli_paged_prompt_logprobs_sink_logits(data, data, data, data, data, data, data, data, data, None, None, 1, 1, 1, B, S, D,
                                                     64, H, Hkv, W, K, z, elem, 0, None, 0, None)


ALL = (_scan, _lean, _prompt, _score)


def test_symbols_are_exported_and_bound_as_the_header_declares_them(mli):
    import inspect
    from min_llm_inference_amd import _lib, engine, ops
    for name in SYMBOLS:
        assert hasattr(mli, name), name
        assert name in _lib.SIGNATURES or name in _lib.ENGINE_SIGNATURES, name
    # the soft-cap entry points argument for argument, a pointer in place of the float
    for name in SYMBOLS[:4]:
        cap = _lib.SIGNATURES[name.replace("sink_logits", "softcap")]
        assert _lib.SIGNATURES[name] == [ctypes.c_void_p if t is ctypes.c_float else t for t in cap], name
        assert cap.count(ctypes.c_float) == 1
    assert _lib.ENGINE_SIGNATURES["mli_engine_set_sink_logits"] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    assert mli.mli_abi_version() == 4          # no existing signature changed
    assert not hasattr(mli, "mli_prompt_scan_tq_sink_logits")        # the variants keep the queries per workgroup
    assert not hasattr(mli, "mli_attention_sink_logits_workspace_bytes")        # the workspace is the multi-head one
    for fn in (ops.decode_scan_paged_sink_logits, engine.Engine.set_sink_logits):
        assert callable(fn)
    for fn in (ops.paged_attention_lean, ops.prompt_scan_paged, ops.paged_prompt_logprobs):
        assert inspect.signature(fn).parameters["sink_logits"].default is None
    assert inspect.signature(engine.Engine.__init__).parameters["sink_logits"].default is None
    # the header: every declaration has `const float* sink_logits` where the soft-cap one has `float cap`
    with open(os.path.join(ROOT, "include", "mli_kernels.h")) as f:
        header = f.read()
    for name in SYMBOLS[:4]:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        other = re.search(r"\bint " + name.replace("sink_logits", "softcap") + r"\(([^;]*)\);", header)
        assert decl and other, name
        norm = lambda s: re.sub(r"\s+", " ", s).strip()
        assert norm(decl.group(1)) == norm(other.group(1)).replace("float cap", "const float* sink_logits"), name
        assert len(decl.group(1).split(",")) == len(_lib.SIGNATURES[name]), name
    with open(os.path.join(ROOT, "include", "mli_engine.h")) as f:
        assert "int mli_engine_set_sink_logits(mli_engine* engine, const float* logits_host, int n);" in f.read()
    for family in FAMILIES:
        assert family.decode() in header


def test_the_python_front_end_refuses_the_pairs_before_any_call():
    from min_llm_inference_amd import ops
    for kw in (dict(alibi_slopes=object()), dict(softcap=2.0)):
        with pytest.raises(ValueError, match="not combined"):
            ops.paged_attention_lean(None, None, None, None, None, None, None, None, 0, 64, n_heads=4, sink_logits=object(), **kw)
    with pytest.raises(ValueError, match="not combined"):
        ops.prompt_scan_paged(None, None, [], None, 8, 64, F32, n_heads=4, softcap=2.0, sink_logits=object())
    with pytest.raises(ValueError, match="not combined"):
        ops.paged_prompt_logprobs(None, None, None, None, [], 8, 64, F32, n_heads=4, softcap=2.0, sink_logits=object())


def test_one_head_is_refused(mli):
    for elem in (F32, BF16, FP8):
        for S in (64, 1024):
            for W, K in FORMS:
                for call in ALL:
                    assert call(mli, 8, S, 128, 1, 1, W, K, elem) == BAD_ARG, (call.__name__, S, W, K, elem)


@pytest.mark.parametrize("H,Hkv", [(8, 4), (8, 1), (8, 8), (2, 1), (2, 2)])
def test_fp8_pages_null_pointers_and_negative_sinks_are_refused(mli, H, Hkv):
    for W, K in FORMS:
        for call in ALL:
            assert call(mli, 8, 64, 256, H, Hkv, W, K, FP8) == BAD_ARG, call.__name__
            assert call(mli, 8, 64, 256, H, Hkv, W, K, 3) == BAD_ARG, call.__name__
            for elem in (F32, BF16):
                assert call(mli, 8, 64, 256, H, Hkv, W, K, elem, z=None) == BAD_ARG, call.__name__
                assert call(mli, 8, 1024, 256, H, Hkv, W, K, elem, z=None) == BAD_ARG      # before any workspace is looked at
                assert call(mli, 8, 64, 256, H, Hkv, W, K, elem, data=None) == BAD_ARG, call.__name__
                assert call(mli, 8, 1024, 256, H, Hkv, W, K, elem, data=None) == BAD_ARG, call.__name__
    for elem in (F32, BF16):
        for W in (0, 12, 64):
            for call in ALL:
                assert call(mli, 8, 64, 256, H, Hkv, W, -1, elem) == BAD_ARG, call.__name__
    assert _prompt(mli, 8, 64, 256, H, Hkv, 0, 0, F32, z=None, n_seg=0) == BAD_ARG       # null logits beside nothing to do, too


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
            assert _scan(mli, 8, 1024, D, H, Hkv, W, K, elem) == WORKSPACE, (elem, D, H, Hkv, W, K)
        assert _score(mli, 8, 1024, D, H, Hkv, 0, 0, elem) == WORKSPACE, (elem, D, H, Hkv)     # the scratch, after the arguments
    assert _scan(mli, 8, 1024, 1024, 4, 1, 0, 0, F32) == BAD_ARG          # fp32 rows of more than two lane loads
    assert _scan(mli, 8, 1024, 2048, 8, 1, 0, 0, BF16) == BAD_ARG
    assert _scan(mli, 8, 1024, 128, 8, 8, 0, 0, F32) == BAD_ARG           # head_dim 16
    assert _prompt(mli, 8, 64, 256, 8, 2, 0, 0, F32, n_seg=0) == 0        # no segments: nothing to do
    assert _prompt(mli, 8, 64, 256, 8, 2, 0, 0, F32, n_seg=-1) == BAD_ARG


def test_the_prompt_scan_keeps_its_queries_per_workgroup(mli):
    assert [mli.mli_prompt_scan_tq(D, 4, e) for D, e in ((128, F32), (512, F32), (256, BF16), (1024, BF16))] == [8, 4, 4, 2]


def test_the_launch_families_are_known_and_no_refusal_counts_a_launch(mli):
    n = ctypes.c_ulonglong(99)
    assert mli.mli_launch_counts_reset() == 0
    for family in FAMILIES:
        assert mli.mli_launch_count(family, ctypes.byref(n)) == 0 and n.value == 0
    _scan(mli, 8, 1024, 256, 8, 2, 0, 0, BF16)                            # refused for its workspace: nothing was enqueued
    _scan(mli, 8, 64, 256, 1, 1, 0, 0, BF16)
    _scan(mli, 8, 64, 256, 8, 2, 0, 0, BF16, z=None)
    _lean(mli, 8, 64, 256, 8, 2, 0, 0, FP8)
    _prompt(mli, 8, 64, 256, 1, 1, 0, 0, BF16)
    _prompt(mli, 8, 64, 256, 8, 2, 0, 0, BF16, z=None)
    _score(mli, 8, 64, 256, 8, 2, 0, -1, F32)
    for family in FAMILIES + (b"scan_heads_softcap", b"scan_prompt_softcap", b"scan_heads_window", b"scan_heads_alibi", b"scan_prompt",
                              b"scan_chunked", b"scan_equal_shares", b"latest_compact", b"fill_flat"):
        assert mli.mli_launch_count(family, ctypes.byref(n)) == 0 and n.value == 0, family
    assert mli.mli_launch_count(b"scan_heads_sink_logit", ctypes.byref(n)) != 0          # an unknown family is an error


def test_the_engine_setter_refuses_a_null_handle(mli):
    z = (ctypes.c_float * 4)(0.5, 0.25, 0.0, -1.0)
    for ptr, n in ((z, 4), (None, 0), (z, 0), (z, -1)):
        assert mli.mli_engine_set_sink_logits(None, ptr, n) == -1
        assert b"null argument" in mli.mli_engine_last_error()


C_HOST = r"""
#include <stdio.h>
#include "mli_kernels.h"
#include "mli_engine.h"
int main(void) {
    int (*scan)(const float*, const void* const*, const int*, float*, int, int, int, int, int, int, int, const float*, int, void*,
                size_t, void*) = mli_decode_scan_paged_sink_logits;
    int (*lean)(void* const*, const int*, const void*, const void*, const void*, const int*, float*, float*, int, int, int, int, int,
                int, int, int, const float*, const float*, int, void*, size_t, void*) = mli_paged_attention_lean_sink_logits;
    int (*prompt)(const float*, const void* const*, const int*, const int*, const int*, const int*, float*, int, int, int, int, int,
                  int, int, int, int, int, const float*, int, void*) = mli_prompt_scan_paged_sink_logits;
    int (*score)(const void* const*, const int*, const void*, const float*, const int*, const int*, const int*, const int*, float*,
                 int*, float*, int, int, int, int, int, int, int, int, int, int, int, const float*, int, int, void*, size_t, void*)
        = mli_paged_prompt_logprobs_sink_logits;
    int (*set)(mli_engine*, const float*, int) = mli_engine_set_sink_logits;
    float z[4] = {0.5f, 0.25f, 0.0f, -1.0f};
    float q[1] = {0.0f};
    const void* table[1] = {0};
    int lengths[1] = {0};
    (void)lean; (void)prompt; (void)score; (void)set;
    /* refusals are decided before anything touches a device: one head, then no logits, then the workspace */
    if (scan(q, table, lengths, q, 8, 64, 128, 1, 1, 0, 0, z, MLI_ELEM_F32, 0, 0, 0) != MLI_ERR_BAD_ARG) return 2;
    if (scan(q, table, lengths, q, 8, 64, 128, 4, 2, 0, 0, 0, MLI_ELEM_F32, 0, 0, 0) != MLI_ERR_BAD_ARG) return 3;
    if (scan(q, table, lengths, q, 8, 1024, 128, 4, 2, 0, 0, z, MLI_ELEM_BF16, 0, 0, 0) != MLI_ERR_WORKSPACE) return 4;
    puts("ok");
    return mli_abi_version() == 4 ? 0 : 1;
}
"""


def test_a_plain_c_host_compiles_against_the_headers_and_calls_an_entry_point(mli, tmp_path):
    src = tmp_path / "sink_logits.c"
    src.write_text(C_HOST)
    inc = os.path.join(ROOT, "include")
    libdir = os.path.join(ROOT, "min_llm_inference_amd", "lib")
    assert shutil.which("gcc") and shutil.which("g++")
    for cmd in (["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", inc, str(src)],
                ["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", inc, "-x", "c++", str(src)]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    exe = tmp_path / "sink_logits_host"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", inc, str(src), "-o", str(exe), "-L", libdir, "-lmli_hip",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", (r.returncode, r.stdout, r.stderr)
