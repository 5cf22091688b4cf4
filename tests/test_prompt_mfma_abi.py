"""The prompt scan on matrix instructions at the drop-in boundary, without a GPU: the shape rule at its frontier, the bindings
against the header, the refusals (decided before anything touches a device: the pointers given are addresses nobody follows),
the ValueErrors of ops and the null-engine refusal of the engine's switch."""
import ctypes
import inspect
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, F32, BF16, FP8 = -22, 0, 1, 2
PTR = ctypes.c_void_p(256)
SYMBOLS = ("mli_prompt_scan_mfma_shape_supported", "mli_prompt_scan_mfma_tq", "mli_prompt_scan_paged_mfma",
           "mli_paged_prompt_logprobs_mfma")

# (B, S, D, H, Hkv, elem) -> accepted: the last accepted and the first refused value of every limit
FRONTIER = [
    ((8, 64, 8192, 64, 8, BF16), 1), ((8, 64, 8320, 65, 65, BF16), 0),          # emb_dim 8192 | beyond
    ((8, 64, 2048, 16, 2, BF16), 1), ((8, 64, 2048, 16, 1, BF16), 0),           # g 8 | 16
    ((8, 64, 2048, 16, 16, BF16), 1), ((8, 64, 384, 3, 1, BF16), 0), ((8, 64, 2048, 16, 3, BF16), 0),   # g 1 | g 3 | no divisor
    ((8, 64, 512, 8, 2, BF16), 1), ((8, 64, 512, 4, 2, BF16), 1),               # head_dim 64, 128
    ((8, 64, 512, 16, 2, BF16), 0), ((8, 64, 512, 2, 2, BF16), 0), ((8, 64, 384, 4, 1, BF16), 0),       # head_dim 32, 256, 96
    ((8, 64, 512, 4, 2, F32), 0), ((8, 64, 512, 4, 2, FP8), 0), ((8, 64, 512, 4, 2, 3), 0),             # page types
    ((8, 16, 512, 4, 2, BF16), 1), ((8, 72, 512, 4, 2, BF16), 0), ((8, 0, 512, 4, 2, BF16), 0),         # n_sequence
    ((16384, 64, 256, 2, 2, BF16), 1), ((16385, 64, 256, 2, 2, BF16), 0), ((0, 64, 256, 2, 2, BF16), 0),   # n_batch
    ((8, 64, 512, 0, 0, BF16), 0), ((8, 64, 512, 4, 0, BF16), 0), ((8, 64, 512, 4, 8, BF16), 0),
]
# (D, H, Hkv) -> queries per workgroup: whole 16-column tiles, four at head_dim 64 and two at 128, 16 queries at most
TQ = [((256, 4, 4), 16), ((256, 4, 2), 16), ((512, 8, 2), 16), ((512, 8, 1), 8), ((512, 4, 4), 16), ((512, 4, 2), 16),
      ((512, 4, 1), 8), ((1024, 8, 1), 4), ((2048, 16, 4), 8), ((512, 16, 2), BAD_ARG), ((384, 3, 1), BAD_ARG)]


def _scan(mli, B=8, S=64, D=512, H=8, Hkv=2, W=0, K=0, elem=BF16, n_seg=2, max_count=5, n_q=10, data=PTR):
    return mli.mli_prompt_scan_paged_mfma(data, data, data, data, data, data, data, n_seg, max_count, n_q, B, S, D, H, Hkv, W, K,
                                          elem, None)


def _logprobs(mli, B=8, S=64, D=512, H=8, Hkv=2, W=0, K=0, elem=BF16, n_seg=2, max_count=5, n=10, data=PTR):
    return mli.mli_paged_prompt_logprobs_mfma(data, data, data, data, data, data, data, data, data, None, None, n_seg, max_count, n,
                                              B, S, D, 100, H, Hkv, W, K, elem, 0, data, 1 << 40, None)


@pytest.mark.parametrize("shape,accepted", FRONTIER)
def test_the_shape_rule_at_its_frontier(mli, shape, accepted):
    B, S, D, H, Hkv, elem = shape
    assert mli.mli_prompt_scan_mfma_shape_supported(*shape) == accepted
    if not accepted:
        assert _scan(mli, B, S, D, H, Hkv, elem=elem, max_count=1) == BAD_ARG
        assert _logprobs(mli, B, S, D, H, Hkv, elem=elem, max_count=1) == BAD_ARG


def test_bindings_match_the_header(mli):
    from min_llm_inference_amd import _lib, engine, ops
    for heads, tq in TQ:
        assert mli.mli_prompt_scan_mfma_tq(*heads) == tq, heads
    with open(os.path.join(ROOT, "include", "mli_kernels.h")) as f:
        header = f.read()
    for name in SYMBOLS:
        decl = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert decl and hasattr(mli, name), name
        args = [a.strip() for a in decl.group(1).split(",")]
        want = [ctypes.c_size_t if a.startswith("size_t") else ctypes.c_int if a.startswith("int ") else ctypes.c_void_p for a in args]
        assert _lib.SIGNATURES[name] == want, name
    assert _lib.ENGINE_SIGNATURES["mli_engine_set_prompt_mfma"] == [ctypes.c_void_p, ctypes.c_int]
    assert mli.mli_abi_version() == 4 and '"scan_prompt_mfma"' in header
    assert b"scan_prompt_mfma" in [mli.mli_launch_family_name(i) for i in range(64)]
    assert inspect.signature(engine.Engine.__init__).parameters["prompt_mfma"].default is False


    for kw in (dict(sinks=4, window=8), dict(softcap=2.0), dict(sink_logits=object())):
        with pytest.raises(ValueError, match="not combined"):
            ops.prompt_scan_paged(None, None, None, None, 8, 64, BF16, n_heads=4, mfma=True, **kw)
        with pytest.raises(ValueError, match="not combined"):
            ops.paged_prompt_logprobs(None, None, None, None, None, 8, 64, BF16, n_heads=4, mfma=True, **kw)


def test_refusals_before_any_launch(mli):
    assert mli.mli_launch_counts_reset() == 0
    for call in (_scan, _logprobs):
        assert call(mli, elem=F32) == BAD_ARG and call(mli, elem=FP8) == BAD_ARG
        assert call(mli, W=8, K=4) == BAD_ARG and call(mli, K=1) == BAD_ARG      # sink tokens, with and without a window
        assert call(mli, W=-1) == BAD_ARG and call(mli, n_seg=-1) == BAD_ARG
        assert call(mli, max_count=0) == BAD_ARG and call(mli, max_count=65) == BAD_ARG     # outside 1 .. n_sequence
        assert call(mli, data=None) == BAD_ARG                                   # null pointers
        assert call(mli, n_seg=0) == 0 and call(mli, n_seg=0, max_count=0) == 0  # nothing to do
    assert _scan(mli, n_seg=0, data=None) == 0
    # the grid bound: 2^21 segments * 4 blocks * 2 K/V heads * 256 threads = 2^32 work items (an accepted grid would be launched)
    assert _scan(mli, n_seg=1 << 21, max_count=64) == BAD_ARG
    assert mli.mli_launch_count(b"scan_prompt_mfma", ctypes.byref(n := ctypes.c_ulonglong(7))) == 0 and n.value == 0
    assert mli.mli_engine_set_prompt_mfma(None, 1) == -1                         # the engine switch on a null engine
    assert b"mli_engine_set_prompt_mfma" in mli.mli_engine_last_error()
