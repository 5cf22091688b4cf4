"""CPU-side checks of the log-probability entry points: exported, bound as the headers declare them, and
every refusal of the contract answered before a device pointer is looked at -- so calls with null device pointers can ask.
No kernel is launched here."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, WORKSPACE = -22, -12
KERNEL_ENTRIES = ("mli_sample_tokens_logprobs", "mli_decoder_sampled_logprobs", "mli_paged_decoder_sampled_logprobs")
ENGINE_ENTRIES = ("mli_engine_set_logprobs", "mli_engine_get_finished_logprobs")


def _prototypes(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {n: (0 if a.strip() in ("", "void") else a.count(",") + 1)
            for n, a in re.findall(r"\b(mli_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text)}


def test_the_entry_points_are_declared_exported_and_bound(mli):
    from min_llm_inference_amd import _lib
    kernels, engine = _prototypes("mli_kernels.h"), _prototypes("mli_engine.h")
    for n in KERNEL_ENTRIES:
        assert n in kernels and hasattr(mli, n), n
        assert len(_lib.SIGNATURES[n]) == kernels[n], (n, kernels[n])
    for n in ENGINE_ENTRIES:
        assert n in engine and hasattr(mli, n), n
        assert len(_lib.ENGINE_SIGNATURES[n]) == engine[n], (n, engine[n])
    text = open(os.path.join(ROOT, "include", "mli_kernels.h")).read()
    assert re.search(r"#define\s+MLI_MAX_TOP_LOGPROBS\s+8\b", text)
    assert mli.mli_abi_version() == 4          # additive: the version of the existing entry points stands
    assert "logprob" in open(os.path.join(ROOT, "include", "mli_shard.h")).read()   # the group says it has none


def _calls(mli, lp, ids, tops, n_top, n_batch=8, n_vocab=1024, emb_dim=128, scratch=None, scratch_bytes=0):
    """the three entry points with null device pointers everywhere but the figures' own arguments"""
    z = None
    return {
        "mli_sample_tokens_logprobs": mli.mli_sample_tokens_logprobs(z, z, z, z, z, z, z, lp, ids, tops, n_batch, n_vocab, n_top,
                                                                    scratch, scratch_bytes, z),
        "mli_decoder_sampled_logprobs": mli.mli_decoder_sampled_logprobs(z, z, z, z, z, z, n_batch, n_vocab, 128, emb_dim, 2, 1,
                                                                        z, z, z, z, lp, ids, tops, n_top, scratch, scratch_bytes, z),
        "mli_paged_decoder_sampled_logprobs": mli.mli_paged_decoder_sampled_logprobs(z, z, z, z, z, z, n_batch, n_vocab, 128,
                                                                                    emb_dim, 2, 1, 0, z, z, z, z, lp, ids, tops,
                                                                                    n_top, scratch, scratch_bytes, z),
    }


@pytest.fixture()
def host_words():
    """three addresses that are not null (host memory: a refusal must come before any of them is followed)"""
    keep = [(ctypes.c_float * 64)(), (ctypes.c_int * 64)(), (ctypes.c_float * 64)()]
    return [ctypes.cast(k, ctypes.c_void_p) for k in keep], keep


@pytest.mark.parametrize("case", ["n_top < 0", "n_top > 8", "null token_logprob", "null top_ids", "null top_logprobs",
                                  "null token_logprob, n_top 0"])
def test_the_logprob_refusals_come_first(mli, host_words, case):
    (lp, ids, tops), _keep = host_words
    args = {"n_top < 0": (lp, ids, tops, -1), "n_top > 8": (lp, ids, tops, 9), "null token_logprob": (None, ids, tops, 3),
            "null top_ids": (lp, None, tops, 3), "null top_logprobs": (lp, ids, None, 1),
            "null token_logprob, n_top 0": (None, None, None, 0)}[case]
    for name, rc in _calls(mli, *args).items():
        assert rc == BAD_ARG, (case, name, rc)


def test_the_refusals_of_the_plain_sampled_entries_carry_over(mli, host_words):
    (lp, ids, tops), _keep = host_words
    for n_top, i, t in ((0, None, None), (8, ids, tops)):            # well-formed figures: the plain refusals answer
        for name, rc in _calls(mli, lp, i, t, n_top, n_batch=0).items():
            assert rc == BAD_ARG, (name, "n_batch 0", rc)
        for name, rc in _calls(mli, lp, i, t, n_top, n_vocab=0).items():
            assert rc == BAD_ARG, (name, "n_vocab 0", rc)
        got = _calls(mli, lp, i, t, n_top, emb_dim=126)
        assert got["mli_decoder_sampled_logprobs"] == BAD_ARG and got["mli_paged_decoder_sampled_logprobs"] == BAD_ARG
        got = _calls(mli, lp, i, t, n_top)                            # no scratch for the logits
        assert got["mli_decoder_sampled_logprobs"] == WORKSPACE and got["mli_paged_decoder_sampled_logprobs"] == WORKSPACE
    z = None
    assert mli.mli_paged_decoder_sampled_logprobs(z, z, z, z, z, z, 8, 1024, 128, 128, 2, 2, 0, z, z, z, z, lp, ids, tops, 3,
                                                  z, 0, z) == BAD_ARG       # i_decoder out of range
    assert mli.mli_paged_decoder_sampled_logprobs(z, z, z, z, z, z, 8, 1024, 128, 128, 2, 1, 3, z, z, z, z, lp, ids, tops, 3,
                                                  z, 0, z) == BAD_ARG       # no such element type
    assert mli.mli_paged_decoder_sampled_logprobs(z, z, z, z, z, z, 8, 1024, 120, 128, 2, 1, 0, z, z, z, z, lp, ids, tops, 3,
                                                  z, 0, z) == BAD_ARG       # n_sequence no multiple of the page


def test_the_engine_entries_follow_the_error_convention_on_a_null_handle(mli):
    n_prompt, n = ctypes.c_int(), ctypes.c_int()
    assert mli.mli_engine_set_logprobs(None, 3) == -1
    assert mli.mli_engine_last_error()
    assert mli.mli_engine_get_finished_logprobs(None, 0, ctypes.byref(n_prompt), None, 0, ctypes.byref(n), None, None, 0) == -1
    assert mli.mli_engine_last_error()
