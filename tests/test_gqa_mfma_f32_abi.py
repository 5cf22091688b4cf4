"""The MFMA grouped-query scan over fp32 pages at the C boundary, without a GPU: the shape rule at the last accepted and the first
refused value of every limit, and the refusals, decided before anything touches a device (nobody follows the pointers)."""
import ctypes

import pytest

BAD_ARG, WORKSPACE, PTR = -22, -12, ctypes.c_void_p(256)

FRONTIER = [   # (B, S, D, H, Hkv), accepted
    ((8, 64, 2048, 16, 2), 1), ((8, 64, 2048, 32, 4), 1), ((8, 64, 2112, 33, 11), 0), ((8, 64, 2176, 17, 17), 0),   # emb_dim 2048 | beyond
    ((8, 64, 1024, 8, 1), 1), ((8, 64, 1152, 9, 1), 0),                         # g 8 | 9
    ((8, 64, 2048, 16, 16), 1), ((8, 64, 2048, 16, 3), 0),                      # g 1 | n_kv_heads no divisor
    ((8, 64, 448, 7, 1), 1), ((8, 64, 2048, 16, 32), 0),                        # odd g | more K/V heads than heads
    ((8, 64, 512, 8, 2), 1), ((8, 64, 512, 4, 2), 1),                           # head_dim 64, 128
    ((8, 64, 512, 16, 2), 0), ((8, 64, 512, 2, 2), 0), ((8, 64, 480, 5, 1), 0),   # head_dim 32, 256, 96
    ((8, 16, 512, 4, 2), 1), ((8, 72, 512, 4, 2), 0), ((8, 0, 512, 4, 2), 0),   # n_sequence
    ((8192, 64, 256, 2, 2), 1), ((8193, 64, 256, 2, 2), 0),                     # B * Hkv <= 16384
    ((1, 262144, 128, 1, 1), 1), ((1, 262160, 128, 1, 1), 0),                   # g 1: 4096 items of 64 tokens | beyond
    ((1, 2097152, 256, 2, 1), 1), ((1, 2097168, 256, 2, 1), 0),                 # g 2: 2048 items of 1024 tokens | beyond
    ((0, 64, 512, 4, 2), 0), ((8, 64, 512, 0, 0), 0), ((8, 64, 512, 4, 0), 0),
]


def _scan(mli, B, S, D, H, Hkv, W=0, data=PTR, ws=None, ws_bytes=0):
    return mli.mli_decode_scan_paged_gqa_mfma_f32(data, data, data, data, B, S, D, H, Hkv, W, ws, ws_bytes, None)


def _lean(mli, B, S, D, H, Hkv, W=0, K=0, data=PTR, w=PTR):
    return mli.mli_paged_attention_lean_gqa_mfma_f32(data, data, w, w, w, None, data, data, B, S, D, 0, H, Hkv, W, K, None, None, 0, None)


@pytest.mark.parametrize("shape,accepted", FRONTIER)
def test_the_f32_shape_rule_at_its_frontier(mli, shape, accepted):
    assert mli.mli_launch_counts_reset() == 0
    assert mli.mli_gqa_mfma_f32_shape_supported(*shape) == accepted
    if accepted:     # a subset of the bf16 rule, whose workspace it uses
        assert mli.mli_gqa_mfma_shape_supported(*shape, 1) == 1 and mli.mli_gqa_mfma_workspace_bytes(*shape) > 65536
    else:
        assert _scan(mli, *shape) == BAD_ARG and _lean(mli, *shape) == BAD_ARG
    assert mli.mli_launch_count(b"scan_gqa_mfma_f32", ctypes.byref(n := ctypes.c_ulonglong(7))) == 0 and n.value == 0


def test_refusals_and_the_workspace(mli):
    assert mli.mli_launch_counts_reset() == 0
    for S in (64, 1024):
        assert _scan(mli, 8, S, 2048, 16, 4, data=None) == BAD_ARG            # a null data pointer, before any workspace is looked at
        assert _lean(mli, 8, S, 2048, 16, 4, data=None) == BAD_ARG
        assert _lean(mli, 8, S, 2048, 16, 4, w=None) == BAD_ARG               # a null weight
        assert _lean(mli, 8, S, 2048, 16, 4, W=8, K=4) == BAD_ARG             # sink tokens
        assert _lean(mli, 8, S, 4096, 32, 8) == BAD_ARG                       # a width the bf16 call takes
    for W in (0, 513):                                                        # several items per row
        assert _scan(mli, 8, 1024, 2048, 16, 4, W) == WORKSPACE
        assert _scan(mli, 8, 1024, 2048, 16, 4, W, ws=PTR, ws_bytes=65536 + 4096) == WORKSPACE
    assert mli.mli_launch_count(b"scan_gqa_mfma_f32", ctypes.byref(n := ctypes.c_ulonglong(7))) == 0 and n.value == 0
    assert mli.mli_engine_set_heads_mfma_f32(None, 16, 4) == -1 and b"null argument" in mli.mli_engine_last_error()
    assert mli.mli_gqa_mfma_shape_supported(8, 64, 2048, 16, 4, 0) == 0      # the existing names keep refusing fp32 pages (elem 0)
    assert mli.mli_paged_attention_lean_gqa_mfma(PTR, PTR, PTR, PTR, PTR, None, PTR, PTR, 8, 64, 2048, 0, 16, 4, 0, 0, None, 0, None, 0, None) == BAD_ARG
