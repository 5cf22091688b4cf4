"""The prompt log-probability entry points at the drop-in boundary, without a GPU: the symbols exist and are bound,
the ABI version is unchanged, and every refusal is answered before anything touches a device -- null device pointers
everywhere, so a call that got past its checks would fault.  n_seg == 0 is a no-op returning 0 for an accepted shape, which
is how an accepted shape is told from a refused one here: fp8 pages, every shape the predicate refuses (against a table),
n_top outside 0 .. 8, null outputs, negative window or sinks; then the engine refusals that need no device."""
import ctypes

import pytest

BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
SYMBOLS = ("mli_prompt_scan_tq", "mli_prompt_scan_paged", "mli_prompt_project_q", "mli_score_tokens_logprobs",
           "mli_prompt_logprobs_scratch_bytes", "mli_paged_prompt_logprobs")
ENGINE_SYMBOLS = ("mli_engine_set_prompt_logprobs", "mli_engine_get_finished_prompt_logprobs")

# (n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, elem) -> accepted
SHAPES = [
    ((8, 128, 64, 1, 1, F32), True), ((8, 128, 512, 1, 1, F32), True), ((8, 128, 516, 1, 1, F32), False),
    ((8, 128, 1024, 1, 1, F32), False), ((8, 128, 1024, 1, 1, BF16), True), ((8, 128, 1032, 1, 1, BF16), False),
    ((8, 128, 2048, 1, 1, BF16), False), ((8, 128, 66, 1, 1, F32), False), ((8, 128, 132, 1, 1, BF16), False),
    ((8, 120, 128, 1, 1, F32), False), ((0, 128, 128, 1, 1, F32), False), ((16385, 128, 128, 1, 1, F32), False),
    ((16384, 128, 128, 1, 1, F32), True), ((8, 0, 128, 1, 1, F32), False),
    ((8, 128, 128, 4, 4, F32), True), ((8, 128, 256, 4, 4, BF16), True), ((8, 128, 64, 4, 4, F32), False),       # head_dim 16
    ((8, 128, 192, 3, 3, F32), True), ((8, 128, 130, 2, 2, F32), False), ((8, 128, 1024, 8, 8, F32), False),
    ((8, 128, 1024, 8, 2, BF16), True), ((8, 128, 256, 8, 1, F32), True), ((8, 128, 256, 8, 3, F32), False),
    ((8, 128, 256, 8, 16, F32), False), ((8, 128, 256, 8, 0, F32), False), ((8, 128, 256, 0, 1, F32), False),
    ((8, 128, 256, 1, 2, F32), False), ((8, 128, 256, -1, -1, F32), False),
    ((8, 128, 256, 1, 1, FP8), False), ((8, 128, 256, 4, 4, FP8), False), ((8, 128, 256, 1, 1, 3), False),
    ((8, 128, 256, 1, 1, -1), False),
]


def _scan(mli, shape, n_seg=0, window=0, sinks=0, max_count=1, n_q=1):
    B, S, D, H, Hkv, elem = shape
    return mli.mli_prompt_scan_paged(None, None, None, None, None, None, None, n_seg, max_count, n_q, B, S, D, H, Hkv, window,
                                     sinks, elem, None)


def _whole(mli, shape, lp, ids, tops, n_top, n_seg=0, window=0, sinks=0, n_vocab=1024, scratch=None, scratch_bytes=0,
           max_count=1, n_positions=1):
    B, S, D, H, Hkv, elem = shape
    return mli.mli_paged_prompt_logprobs(None, None, None, None, None, None, None, None, lp, ids, tops, n_seg, max_count,
                                         n_positions, B, S, D, n_vocab, H, Hkv, window, sinks, elem, n_top, scratch,
                                         scratch_bytes, None)


@pytest.fixture()
def host_words():
    """three addresses that are not null (host memory: a refusal must come before any of them is followed)"""
    keep = [(ctypes.c_float * 64)(), (ctypes.c_int * 64)(), (ctypes.c_float * 64)()]
    return [ctypes.cast(k, ctypes.c_void_p) for k in keep], keep


def test_symbols_are_exported_and_bound(mli):
    from min_llm_inference_amd import _lib
    for name in SYMBOLS:
        assert hasattr(mli, name) and name in _lib.SIGNATURES, name
    for name in ENGINE_SYMBOLS:
        assert hasattr(mli, name) and name in _lib.ENGINE_SIGNATURES, name
    assert mli.mli_abi_version() == 4          # additive: no existing signature changed
    n = ctypes.c_ulonglong(5)
    assert mli.mli_launch_count(b"scan_prompt", ctypes.byref(n)) == 0 and n.value == 0


@pytest.mark.parametrize("shape,accepted", SHAPES)
def test_the_shape_table(mli, host_words, shape, accepted):
    (lp, ids, tops), _keep = host_words
    want = 0 if accepted else BAD_ARG
    assert _scan(mli, shape) == want
    assert _whole(mli, shape, lp, ids, tops, 3) == want
    B, S, D, H, Hkv, elem = shape
    tq = mli.mli_prompt_scan_tq(D, H, elem)
    if accepted:
        assert tq in (2, 4, 8)
        # with segments the null pointers are the next refusal: still nothing is launched
        assert _scan(mli, shape, n_seg=1) == BAD_ARG
    for window, sinks in ((-1, 0), (0, -1), (-5, -5)):
        assert _scan(mli, shape, window=window, sinks=sinks) == BAD_ARG
        assert _whole(mli, shape, lp, ids, tops, 3, window=window, sinks=sinks) == BAD_ARG
    assert _scan(mli, shape, n_seg=-1) == BAD_ARG


def test_windows_and_sinks_of_any_size_are_accepted(mli):
    for window, sinks in ((1, 0), (16, 0), (40, 4), (128, 0), (1 << 30, 1 << 30), (0, 7)):
        assert _scan(mli, (8, 128, 128, 1, 1, F32), window=window, sinks=sinks) == 0
        assert _scan(mli, (8, 128, 256, 8, 2, BF16), window=window, sinks=sinks) == 0


@pytest.mark.parametrize("case", ["n_top < 0", "n_top > 8", "null token_logprob", "null top_ids", "null top_logprobs",
                                  "null token_logprob, n_top 0"])
def test_the_logprob_refusals_come_first(mli, host_words, case):
    (lp, ids, tops), _keep = host_words
    args = {"n_top < 0": (lp, ids, tops, -1), "n_top > 8": (lp, ids, tops, 9), "null token_logprob": (None, ids, tops, 3),
            "null top_ids": (lp, None, tops, 3), "null top_logprobs": (lp, ids, None, 1),
            "null token_logprob, n_top 0": (None, None, None, 0)}[case]
    ok = (8, 128, 128, 1, 1, F32)
    assert _whole(mli, ok, *args) == BAD_ARG
    assert _whole(mli, ok, *args, n_seg=2) == BAD_ARG
    assert mli.mli_score_tokens_logprobs(None, None, *args[:3], 4, 1024, args[3], None) == BAD_ARG
    assert mli.mli_score_tokens_logprobs(None, None, *args[:3], 0, 1024, args[3], None) == BAD_ARG


def test_the_remaining_refusals_and_the_scratch_query(mli, host_words):
    (lp, ids, tops), _keep = host_words
    ok = (8, 128, 128, 1, 1, F32)
    assert mli.mli_score_tokens_logprobs(None, None, lp, ids, tops, 0, 1024, 3, None) == 0        # no rows: a no-op
    assert mli.mli_score_tokens_logprobs(None, None, lp, None, None, 0, 1024, 0, None) == 0
    assert mli.mli_score_tokens_logprobs(None, None, lp, ids, tops, -1, 1024, 3, None) == BAD_ARG
    assert mli.mli_score_tokens_logprobs(None, None, lp, ids, tops, 4, 0, 3, None) == BAD_ARG
    assert mli.mli_score_tokens_logprobs(None, None, lp, ids, tops, 4, 1024, 3, None) == BAD_ARG    # null logits / targets
    assert _whole(mli, ok, lp, ids, tops, 3, n_vocab=0) == BAD_ARG
    for max_count, n_q in ((0, 1), (129, 1), (1, 0)):
        assert _scan(mli, ok, n_seg=1, max_count=max_count, n_q=n_q) == BAD_ARG
        assert _whole(mli, ok, lp, ids, tops, 3, n_seg=1, max_count=max_count, n_positions=n_q) == BAD_ARG
    # mli_prompt_project_q: element types, shapes, no segments, null pointers
    z = None
    assert mli.mli_prompt_project_q(z, z, z, z, z, z, z, z, 0, 1, 1, 8, 128, 128, F32, z) == 0
    assert mli.mli_prompt_project_q(z, z, z, z, z, z, z, z, 0, 1, 1, 8, 128, 128, FP8, z) == BAD_ARG
    assert mli.mli_prompt_project_q(z, z, z, z, z, z, z, z, 0, 1, 1, 8, 128, 132, BF16, z) == BAD_ARG
    assert mli.mli_prompt_project_q(z, z, z, z, z, z, z, z, 0, 1, 1, 8, 120, 128, F32, z) == BAD_ARG
    assert mli.mli_prompt_project_q(z, z, z, z, z, z, z, z, 1, 1, 1, 8, 128, 128, F32, z) == BAD_ARG
    assert mli.mli_prompt_project_q(z, z, z, z, z, z, z, z, -1, 1, 1, 8, 128, 128, F32, z) == BAD_ARG
    # the scratch: [gathered x | q | attention] rows, the logits, the targets, each region padded to 256 bytes
    up = lambda v: (v + 255) & ~255
    for n, D, V in ((8, 128, 1024), (7, 64, 1000), (1, 1024, 50257)):
        assert mli.mli_prompt_logprobs_scratch_bytes(n, D, V) == 3 * up(n * D * 4) + up(n * V * 4) + up(n * 4)
    for bad in ((0, 128, 1024), (8, 0, 1024), (8, 128, 0), (-1, 128, 1024)):
        assert mli.mli_prompt_logprobs_scratch_bytes(*bad) == 0


def test_mli_prompt_scan_tq_refuses_rows_the_scan_does_not_take(mli):
    for D, H, elem in ((516, 1, F32), (1032, 1, BF16), (0, 1, F32), (128, 0, F32), (128, 1, FP8), (66, 1, F32)):
        assert mli.mli_prompt_scan_tq(D, H, elem) == BAD_ARG, (D, H, elem)
    assert mli.mli_prompt_scan_tq(512, 1, F32) == mli.mli_prompt_scan_tq(260, 1, F32)       # one variant: two lane loads


def test_the_engine_entries_follow_the_error_convention_on_a_null_handle(mli):
    n = ctypes.c_int()
    assert mli.mli_engine_set_prompt_logprobs(None, 1) == -1
    assert mli.mli_engine_last_error()
    assert mli.mli_engine_get_finished_prompt_logprobs(None, 0, None, 0, ctypes.byref(n), None, None, 0) == -1
    assert mli.mli_engine_last_error()
