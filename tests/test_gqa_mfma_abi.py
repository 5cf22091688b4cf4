"""The matrix-instruction grouped-query scan at the drop-in boundary, without a GPU: the shape rule by enumeration over its
frontier, the bindings against the header, the refusals (decided before anything touches a device: the pointers given are
addresses nobody follows), and MLI_ERR_WORKSPACE for a shape with several items per row and no workspace."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
PTR = ctypes.c_void_p(256)
SYMBOLS = ("mli_gqa_mfma_shape_supported", "mli_gqa_mfma_workspace_bytes", "mli_decode_scan_paged_gqa_mfma",
           "mli_paged_attention_lean_gqa_mfma")

# (B, S, D, H, Hkv, elem) -> accepted: the last accepted and the first refused value of every limit
FRONTIER = [
    ((8, 64, 8192, 64, 8, BF16), 1), ((8, 64, 8320, 65, 13, BF16), 0),          # emb_dim 8192 | beyond
    ((8, 64, 1024, 8, 1, BF16), 1), ((8, 64, 1152, 9, 1, BF16), 0),             # g 8 | 9
    ((8, 64, 2048, 16, 16, BF16), 1), ((8, 64, 2048, 16, 3, BF16), 0),          # g 1 | n_kv_heads no divisor
    ((8, 64, 448, 7, 1, BF16), 1), ((8, 64, 2048, 16, 32, BF16), 0),            # odd g | more K/V heads than heads
    ((8, 64, 512, 8, 2, BF16), 1), ((8, 64, 512, 4, 2, BF16), 1),               # head_dim 64, 128
    ((8, 64, 512, 16, 2, BF16), 0), ((8, 64, 512, 2, 2, BF16), 0), ((8, 64, 480, 5, 1, BF16), 0),   # head_dim 32, 256, 96
    ((8, 64, 512, 4, 2, F32), 0), ((8, 64, 512, 4, 2, FP8), 0), ((8, 64, 512, 4, 2, 3), 0),         # page types
    ((8, 16, 512, 4, 2, BF16), 1), ((8, 72, 512, 4, 2, BF16), 0), ((8, 0, 512, 4, 2, BF16), 0),     # n_sequence
    ((8192, 64, 256, 2, 2, BF16), 1), ((8193, 64, 256, 2, 2, BF16), 0), ((16384, 64, 256, 2, 1, BF16), 1),   # B * Hkv <= 16384
    ((1, 262144, 128, 1, 1, BF16), 1), ((1, 262160, 128, 1, 1, BF16), 0),       # g 1: items of 64 tokens, 4096 of them | beyond
    ((1, 2097152, 256, 2, 1, BF16), 1), ((1, 2097168, 256, 2, 1, BF16), 0),     # g 2: items grow to 1024 tokens, 2048 of them
    ((0, 64, 512, 4, 2, BF16), 0),((8, 64, 512, 0, 0, BF16), 0), ((8, 64, 512, 4, 0, BF16), 0),
]


def _scan(mli, B, S, D, H, Hkv, W=0, data=PTR, ws=None, ws_bytes=0):
    return mli.mli_decode_scan_paged_gqa_mfma(data, data, data, data, B, S, D, H, Hkv, W, ws, ws_bytes, None)


def _lean(mli, B, S, D, H, Hkv, W=0, K=0, elem=BF16, data=PTR, w=PTR):
    return mli.mli_paged_attention_lean_gqa_mfma(data, data, w, w, w, None, data, data, B, S, D, 0, H, Hkv, W, K, None, elem, None, 0,
                                                 None)


@pytest.mark.parametrize("shape,accepted", FRONTIER)
def test_the_shape_rule_at_its_frontier(mli, shape, accepted):
    B, S, D, H, Hkv, elem = shape
    assert mli.mli_launch_counts_reset() == 0
    assert mli.mli_gqa_mfma_shape_supported(*shape) == accepted
    need = mli.mli_gqa_mfma_workspace_bytes(B, S, D, H, Hkv)
    if elem == BF16:
        assert (need > 65536) == bool(accepted)
    if not accepted:
        if elem == BF16:
            assert _scan(mli, B, S, D, H, Hkv) == BAD_ARG
        assert _lean(mli, B, S, D, H, Hkv, elem=elem) == BAD_ARG
    assert mli.mli_launch_count(b"scan_gqa_mfma", ctypes.byref(n := ctypes.c_ulonglong(7))) == 0 and n.value == 0


def test_bindings_match_the_header(mli):
    import inspect
    from min_llm_inference_amd import _lib, ops
    with open(os.path.join(ROOT, "include", "mli_kernels.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        decl = re.search(r"\b(?:int|size_t) " + name + r"\(([^;]*)\);", header)
        assert decl and hasattr(mli, name), name
        args = [a.strip() for a in decl.group(1).split(",")]
        want = [ctypes.c_size_t if a.startswith("size_t") else ctypes.c_int if a.startswith("int ") else ctypes.c_void_p for a in args]
        assert _lib.SIGNATURES[name] == want, name
    assert getattr(mli, "mli_gqa_mfma_workspace_bytes").restype is ctypes.c_size_t
    assert mli.mli_abi_version() == 4 and "scan_gqa_mfma" in header          # no existing signature changed
    assert callable(ops.decode_scan_paged_gqa_mfma)
    assert inspect.signature(ops.paged_attention_lean).parameters["heads_mfma"].default is False
    for kw in (dict(sinks=4, window=8), dict(alibi_slopes=object()), dict(softcap=2.0), dict(sink_logits=object())):
        with pytest.raises(ValueError, match="not combined"):
            ops.paged_attention_lean(None, None, None, None, None, None, None, None, 0, 64, n_heads=4, heads_mfma=True, **kw)


def test_refusals_and_the_workspace(mli):
    assert mli.mli_launch_counts_reset() == 0
    for S in (64, 1024):
        assert _scan(mli, 8, S, 2048, 16, 4, data=None) == BAD_ARG            # a null data pointer, before any workspace is looked at
        assert _lean(mli, 8, S, 2048, 16, 4, data=None) == BAD_ARG
        assert _lean(mli, 8, S, 2048, 16, 4, w=None) == BAD_ARG               # a null weight
        assert _lean(mli, 8, S, 2048, 16, 4, W=8, K=4) == BAD_ARG             # sink tokens
        for elem in (F32, FP8):
            assert _lean(mli, 8, S, 2048, 16, 4, elem=elem) == BAD_ARG
    # several items per row: without a workspace, and with one a byte short of the need
    need = mli.mli_gqa_mfma_workspace_bytes(8, 1024, 2048, 16, 4)
    assert need == 65536 + 8 * 16 * 16 * 8 + 8 * 16 * 2048 * 4                # counters | (m, l) per (row, 64 tokens, head) | partial rows
    for W in (0, 513):
        assert _scan(mli, 8, 1024, 2048, 16, 4, W) == WORKSPACE
        assert _scan(mli, 8, 1024, 2048, 16, 4, W, ws=PTR, ws_bytes=65536 + 4096) == WORKSPACE
    assert mli.mli_launch_count(b"scan_gqa_mfma", ctypes.byref(n := ctypes.c_ulonglong(7))) == 0 and n.value == 0
