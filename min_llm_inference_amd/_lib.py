"""ctypes loader for libmli_hip.so (C ABI: include/mli_kernels.h, include/mli_engine.h, include/mli_shard.h)."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class MliError(RuntimeError):
    """Raised when a C-ABI call returns non-zero (the reference throws std::runtime_error("Cuda Failure"))."""


def library_path():
    return os.path.join(_HERE, "lib", "libmli_hip.so")


def load_library():
    """Load the HIP library.  There is deliberately no fallback: a missing .so is a hard error."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # torch bundles its own libamdhip64 / libhsa-runtime64.  Import it FIRST so that libmli_hip.so's
    # libamdhip64.so.7 dependency resolves to the copy already in the process; loading /opt/rocm's runtime
    # beside torch's gives two HSA runtimes in one process, and the second one to initialise sees no GPU.
    import torch  # noqa: F401
    path = library_path()
    if not os.path.exists(path):
        raise MliError(
            f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the product path.")
    lib = ctypes.CDLL(path)
    _declare(lib)
    _LIB = lib
    return lib


_P = ctypes.c_void_p
_I = ctypes.c_int
_Z = ctypes.c_size_t

# name -> argtypes; restype is int unless listed in _RESTYPES.  Mirrors include/mli_kernels.h 1:1.
SIGNATURES = {
    "mli_abi_version": [],
    "mli_elem_supported": [_I],
    "mli_attention_workspace_bytes": [_I, _I, _I],
    "mli_attention_workspace_init": [_P, _Z, _P],
    "mli_fill_new_kt_v_cache": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "mli_get_latest_kt_q_v": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "mli_qkt": [_P, _P, _P, _P, _I, _I, _I, _P],
    "mli_softmax_in_place_with_lengths": [_P, _P, _I, _I, _P],
    "mli_softmax_v": [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P],
    "mli_inference_self_attention": [_P] * 11 + [_I] * 5 + [_P, _Z, _P],
    "mli_fill_new_k_v_cache_paged": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "mli_get_latest_k_q_v_paged": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "mli_qkt_paged": [_P, _P, _P, _P, _I, _I, _I, _P],
    "mli_softmax_v_paged": [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P],
    "mli_paged_attention": [_P] * 9 + [_I] * 4 + [_P, _Z, _P],
    "mli_fill_new_k_v_cache_paged_bf16": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    "mli_get_latest_k_q_v_paged_bf16": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    "mli_qkt_paged_bf16": [_P, _P, _P, _P, _I, _I, _I, _P],
    "mli_softmax_v_paged_bf16": [_P, _P, _P, _P, _I, _I, _I, _P, _Z, _P],
    "mli_paged_attention_bf16": [_P] * 9 + [_I] * 4 + [_P, _Z, _P],
    "mli_paged_attention_encoder_bf16": [_P] * 6 + [_I] * 4 + [_P],
    "mli_paged_decoder_multi_rounds_bf16": [_P] * 7 + [_I] * 6 + [_P],
    "mli_decode_scan_paged": [_P] * 5 + [_I] * 5 + [_P, _Z, _P],
    "mli_paged_attention_lean": [_P] * 8 + [_I] * 5 + [_P, _Z, _P],
    "mli_attention_heads_workspace_bytes": [_I, _I, _I, _I],
    "mli_decode_scan_paged_heads": [_P] * 4 + [_I] * 5 + [_P, _Z, _P],
    "mli_paged_attention_lean_heads": [_P] * 8 + [_I] * 6 + [_P, _Z, _P],
    "mli_decode_scan_paged_window": [_P] * 4 + [_I] * 6 + [_P, _Z, _P],
    "mli_paged_attention_lean_window": [_P] * 8 + [_I] * 7 + [_P, _Z, _P],
    "mli_decode_scan_paged_sinks": [_P] * 4 + [_I] * 7 + [_P, _Z, _P],
    "mli_paged_attention_lean_sinks": [_P] * 8 + [_I] * 8 + [_P, _Z, _P],
    "mli_decode_scan_paged_gqa": [_P] * 4 + [_I] * 8 + [_P, _Z, _P],
    "mli_paged_attention_lean_gqa": [_P] * 8 + [_I] * 9 + [_P, _Z, _P],
    "mli_decode_scan_paged_alibi": [_P] * 4 + [_I] * 7 + [_P, _I, _P, _Z, _P],
    "mli_paged_attention_lean_alibi": [_P] * 8 + [_I] * 8 + [_P, _I, _P, _Z, _P],
    "mli_alibi_slopes": [_I, _P],
    "mli_decode_scan_paged_softcap": [_P] * 4 + [_I] * 7 + [ctypes.c_float, _I, _P, _Z, _P],
    "mli_paged_attention_lean_softcap": [_P] * 8 + [_I] * 8 + [ctypes.c_float, _P, _I, _P, _Z, _P],
    "mli_decode_scan_paged_sink_logits": [_P] * 4 + [_I] * 7 + [_P, _I, _P, _Z, _P],
    "mli_paged_attention_lean_sink_logits": [_P] * 8 + [_I] * 8 + [_P, _P, _I, _P, _Z, _P],
    "mli_rope_table": [_I, _I, ctypes.c_double, _P],
    "mli_get_latest_k_q_v_paged_rope": [_P] * 6 + [_I] * 4 + [_P, _I, _P],
    "mli_fill_new_k_v_cache_paged_rope": [_P] * 5 + [_I] * 5 + [_P, _I, _P],
    "mli_paged_prefill_rope": [_P] * 8 + [_I] * 7 + [_P, _I, _P],
    "mli_paged_attention_lean_rope": [_P] * 8 + [_I] * 8 + [_P, _P, _I, _P, _Z, _P],
    "mli_get_latest_k_q_v_paged_lean": [_P] * 6 + [_I] * 4 + [_P],
    "mli_self_attention_lean": [_P] * 10 + [_I] * 5 + [_P, _Z, _P],
    "mli_decode_scan_contiguous": [_P] * 5 + [_I] * 3 + [_P, _Z, _P],
    "mli_decoder_scratch_bytes": [_I, _I],
    "mli_decoder_fused": [_P] * 6 + [_I] * 4 + [_P, _Z, _P],
    "mli_paged_decoder_fused": [_P] * 6 + [_I] * 7 + [_P, _Z, _P],
    "mli_sample_scratch_bytes": [_I, _I],
    "mli_sample_tokens": [_P] * 7 + [_I] * 2 + [_P, _Z, _P],
    "mli_decoder_sampled_scratch_bytes": [_I, _I],
    "mli_decoder_sampled": [_P] * 6 + [_I] * 4 + [_P] * 4 + [_P, _Z, _P],
    "mli_paged_decoder_sampled": [_P] * 6 + [_I] * 7 + [_P] * 4 + [_P, _Z, _P],
    "mli_sample_tokens_logprobs": [_P] * 10 + [_I] * 3 + [_P, _Z, _P],
    "mli_decoder_sampled_logprobs": [_P] * 6 + [_I] * 6 + [_P] * 7 + [_I] + [_P, _Z, _P],
    "mli_paged_decoder_sampled_logprobs": [_P] * 6 + [_I] * 7 + [_P] * 7 + [_I] + [_P, _Z, _P],
    "mli_prompt_scan_tq": [_I, _I, _I],
    "mli_prompt_scan_paged": [_P] * 7 + [_I] * 11 + [_P],
    "mli_prompt_project_q": [_P] * 8 + [_I] * 7 + [_P],
    "mli_score_tokens_logprobs": [_P] * 5 + [_I] * 3 + [_P],
    "mli_prompt_logprobs_scratch_bytes": [_I, _I, _I],
    "mli_paged_prompt_logprobs": [_P] * 11 + [_I] * 13 + [_P, _Z, _P],
    "mli_prompt_scan_paged_softcap": [_P] * 7 + [_I] * 10 + [ctypes.c_float, _I, _P],
    "mli_paged_prompt_logprobs_softcap": [_P] * 11 + [_I] * 11 + [ctypes.c_float, _I, _I, _P, _Z, _P],
    "mli_prompt_scan_paged_sink_logits": [_P] * 7 + [_I] * 10 + [_P, _I, _P],
    "mli_paged_prompt_logprobs_sink_logits": [_P] * 11 + [_I] * 11 + [_P, _I, _I, _P, _Z, _P],
    "mli_paged_prefill": [_P] * 8 + [_I] * 5 + [_P],
    "mli_paged_prefill_window": [_P] * 8 + [_I] * 7 + [_P],
    "mli_prefill": [_P] * 10 + [_I] * 5 + [_P],
    "mli_paged_decode_step": [_P] * 10 + [_I] * 7 + [_P, _Z, _P, _Z, _P],
    "mli_decode_step": [_P] * 13 + [_I] * 4 + [_P, _Z, _P, _Z, _P],
    "mli_graph_begin_capture": [_P],
    "mli_graph_end_capture": [_P, ctypes.POINTER(ctypes.c_void_p)],
    "mli_graph_launch": [_P, _P],
    "mli_stream_wait_stream": [_P, _P],
    "mli_graph_destroy": [_P],
    "mli_inference_optimized_encoder": [_P] * 6 + [_I] * 4 + [_P],
    "mli_paged_attention_encoder": [_P] * 6 + [_I] * 4 + [_P],
    "mli_decoder": [_P] * 7 + [_I] * 4 + [_P],
    "mli_paged_decoder_multi_rounds": [_P] * 7 + [_I] * 6 + [_P],
    "mli_clone_inp_embedding_k_v_cache": [_P] * 5 + [_I] * 3 + [_P],
    "mli_tune": [ctypes.c_char_p, _I],
    "mli_launch_count": [ctypes.c_char_p, ctypes.POINTER(ctypes.c_ulonglong)],
    "mli_launch_counts_reset": [],
    "mli_scan_resident_threshold": [ctypes.c_longlong, _I, _I, _I],
    "mli_scan_resident_keeps": [_P, _I],
    "mli_stream_copy": [_P, _P, _Z, _P],
    "mli_stream_read": [_P, _P, _Z, _P],
    "mli_f32_to_fp8": [_P, _P, _Z, _P],
}
class EngineConfig(ctypes.Structure):
    """mli_engine_config (include/mli_engine.h)."""
    _fields_ = [("kind", _I), ("n_batch", _I), ("n_sequence", _I), ("emb_dim", _I), ("n_vocab", _I),
                ("n_blocks", _I), ("n_forward_rounds", _I), ("device", _I), ("reference_length_reset_quirk", _I)]


class EngineStats(ctypes.Structure):
    """mli_engine_stats (include/mli_engine.h)."""
    _fields_ = [("total_tokens", ctypes.c_longlong), ("seconds", ctypes.c_double), ("iterations", ctypes.c_longlong),
                ("finished", _I), ("waiting", _I), ("in_flight", _I)]


class EnginePageStats(ctypes.Structure):
    """mli_engine_page_stats (include/mli_engine.h)."""
    _fields_ = [("pool_pages", _I), ("in_use", _I), ("peak_in_use", _I), ("released_early", ctypes.c_longlong),
                ("preemptions", ctypes.c_longlong)]


_PP = ctypes.POINTER(ctypes.c_void_p)
_IP = ctypes.POINTER(_I)
ENGINE_SIGNATURES = {
    "mli_engine_create": [ctypes.POINTER(EngineConfig), _P, _P, _P, _P, _P, _PP],
    "mli_engine_destroy": [_P],
    "mli_engine_add_item": [_P, _I, _P, _I],
    "mli_engine_add_item_sampled": [_P, _I, _P, _I, ctypes.c_float, _I, ctypes.c_float, ctypes.c_ulonglong],
    "mli_engine_use_private_stream": [_P],
    "mli_engine_set_pipelined": [_P, _I],
    "mli_engine_run": [_P, ctypes.POINTER(EngineStats)],
    "mli_engine_step": [_P, _IP],
    "mli_engine_get_stats": [_P, ctypes.POINTER(EngineStats)],
    "mli_engine_decoder_result": [_P, _PP, _IP],
    "mli_engine_get_finished": [_P, _I, _IP, _P, _I, _IP],
    "mli_engine_set_logprobs": [_P, _I],
    "mli_engine_get_finished_logprobs": [_P, _I, _IP, _P, _I, _IP, _P, _P, _I],
    "mli_engine_set_prompt_logprobs": [_P, _I],
    "mli_engine_get_finished_prompt_logprobs": [_P, _I, _P, _I, _IP, _P, _P, _I],
    "mli_engine_configure": [_P, _I, _I],
    "mli_engine_set_heads": [_P, _I],
    "mli_engine_set_window": [_P, _I],
    "mli_engine_set_sinks": [_P, _I],
    "mli_engine_set_kv_heads": [_P, _I],
    "mli_engine_set_alibi": [_P, _P, _I],
    "mli_engine_set_softcap": [_P, ctypes.c_float],
    "mli_engine_set_sink_logits": [_P, _P, _I],
    "mli_engine_set_rope": [_P, ctypes.c_double],
    "mli_engine_set_rope_table": [_P, _P, _Z],
    "mli_engine_set_page_release": [_P, _I],
    "mli_engine_get_page_stats": [_P, ctypes.POINTER(EnginePageStats)],
    "mli_engine_set_lean_layers": [_I],
    "mli_engine_set_step_graphs": [_I],
    "mli_engine_last_error": [],
    "mli_engine_stream": [_P, _PP],
    # include/mli_shard.h: the row-sharded engine group (one engine per GPU, RCCL all-gather of the token ids)
    "mli_shard_group_create": [ctypes.POINTER(EngineConfig), _I, _P, _P, _P, _P, _P, _P, _PP],
    "mli_shard_group_create_loopback": [ctypes.POINTER(EngineConfig), _I, _I, _P, _P, _P, _P, _P, _PP],
    "mli_shard_group_destroy": [_P],
    "mli_shard_group_size": [_P],
    "mli_shard_group_add_item": [_P, _I, _P, _I],
    "mli_shard_group_run": [_P, _P],
    "mli_shard_group_gathered": [_P, _I, _PP, _IP],
    "mli_shard_group_engine": [_P, _I],
    "mli_shard_last_error": [],
}


class ShardStats(ctypes.Structure):
    """mli_shard_stats (include/mli_shard.h)."""
    _fields_ = [("total_tokens", ctypes.c_longlong), ("seconds", ctypes.c_double), ("iterations", ctypes.c_longlong),
                ("finished", _I), ("ranks_seen", _I), ("gather_us", ctypes.c_double)]


_RESTYPES = {"mli_shard_last_error": ctypes.c_char_p, "mli_shard_group_destroy": None, "mli_shard_group_engine": _P,
             "mli_attention_workspace_bytes": _Z, "mli_attention_heads_workspace_bytes": _Z,
             "mli_decoder_scratch_bytes": _Z, "mli_prompt_logprobs_scratch_bytes": _Z,
             "mli_sample_scratch_bytes": _Z, "mli_decoder_sampled_scratch_bytes": _Z, "mli_engine_last_error": ctypes.c_char_p,
             "mli_engine_destroy": None, "mli_engine_set_lean_layers": None,
             "mli_engine_set_step_graphs": None}


def _declare(lib):
    for name, argtypes in list(SIGNATURES.items()) + list(ENGINE_SIGNATURES.items()):
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch: fail loudly
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, _I)
