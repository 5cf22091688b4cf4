"""torch-tensor front end over the C ABI, one function per reference launcher (same names).

torch supplies device memory and the stream only; every computation happens in libmli_hip.so.
Argument order and meaning follow the reference headers
(include/kernels/self_attention_inference_optimized.h, include/kernels/paged_attention.h,
include/kernels/encoder.h, include/kernels/decoder.h); scalars the reference derives from
Tensor shapes are derived from the torch shapes here in the same way.
"""
import ctypes

import numpy as np
import torch

from ._lib import MliError, load_library  # noqa: F401  (re-exported: ops.MliError, ops.load_library)

PAGE_BLOCK_SIZE = 16
EMPTY_ROW_TOKEN_ID = -1
EOF_TOKEN_ID = 1023

ELEM_F32, ELEM_BF16, ELEM_FP8 = 0, 1, 2  # MLI_ELEM_* of include/mli_kernels.h

_workspaces = {}


def has_fp8():
    """Whether this build of the library implements the fp8 (OCP e4m3) page extension."""
    return bool(load_library().mli_elem_supported(ELEM_FP8))


def _p(t):
    if t is None:
        return ctypes.c_void_p(0)
    if not t.is_cuda:
        raise MliError("libmli_hip.so operates on device tensors only (no CPU fallback)")
    if not t.is_contiguous():
        raise MliError("tensors crossing the C ABI must be contiguous")
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc, what):
    if rc != 0:
        raise MliError(f"Hip Failure: {what} returned {rc}")


def launch_count(family):
    """How many launches of the kernel family (or form) `family` the calling thread has enqueued since its last
    reset_launch_counts(): mli_launch_count of include/mli_kernels.h, which lists the names."""
    n = ctypes.c_ulonglong(0)
    name = family.encode() if isinstance(family, str) else family
    _check(load_library().mli_launch_count(name, ctypes.byref(n)), f"mli_launch_count({family!r})")
    return int(n.value)


def reset_launch_counts():
    """Zero the calling thread's launch counters (mli_launch_counts_reset)."""
    _check(load_library().mli_launch_counts_reset(), "mli_launch_counts_reset")


def workspace_for(n_batch, n_sequence, dim, device, n_heads=1):
    """Caller-owned scratch for the split-sequence kernels (grown on demand, never inside a timed region).  n_heads > 1:
    sized for the multi-head scan (mli_attention_heads_workspace_bytes), which covers the single-head calls too."""
    lib = load_library()
    if n_heads == 1:
        need = int(lib.mli_attention_workspace_bytes(n_batch, n_sequence, dim))
    else:
        need = int(lib.mli_attention_heads_workspace_bytes(n_batch, n_sequence, dim, int(n_heads)))
    # one buffer per (device, stream), as the C++ side keys its scratch (host/src/memory_hip.cpp): the split-sequence
    # kernels of two streams must not share partial sums.  A buffer that has to grow is replaced only after the
    # stream that used the old one has drained.
    index = device.index if device.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(index)
    key = (index, stream.cuda_stream)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < need:
        if ws is not None:
            stream.synchronize()
        ws = torch.zeros(max(need, 16), dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws, need


# ---- contiguous ("naive") path ------------------------------------------------------------
def launch_fill_new_kt_v_cache(inp_embedding, new_batch_idx, lengths, wk, wv, kt_cache, v_cache, n_new_items):
    B, S, Din = inp_embedding.shape
    _check(load_library().mli_fill_new_kt_v_cache(_p(inp_embedding), _p(new_batch_idx), _p(lengths), _p(wk), _p(wv),
                                                  _p(kt_cache), _p(v_cache), B, S, Din, wk.shape[1], n_new_items,
                                                  _stream()), "mli_fill_new_kt_v_cache")


def launch_get_latest_kt_q_v(inp_embedding, lengths, wk, wq, wv, kt_cache, v_cache, q_output):
    B, S, Din = inp_embedding.shape
    _check(load_library().mli_get_latest_kt_q_v(_p(inp_embedding), _p(lengths), _p(wk), _p(wq), _p(wv), _p(kt_cache),
                                                _p(v_cache), _p(q_output), B, S, Din, wk.shape[1], _stream()),
           "mli_get_latest_kt_q_v")


def launch_qkt(q_output, kt_cache, lengths, qkt_output):
    B, D = q_output.shape
    _check(load_library().mli_qkt(_p(q_output), _p(kt_cache), _p(lengths), _p(qkt_output), B, kt_cache.shape[2], D,
                                  _stream()), "mli_qkt")


def launch_softmax_in_place_with_lengths(qkt_output, lengths):
    B, S = qkt_output.shape
    _check(load_library().mli_softmax_in_place_with_lengths(_p(qkt_output), _p(lengths), B, S, _stream()),
           "mli_softmax_in_place_with_lengths")


def launch_softmax_v(softmax_result, v_cache, attention_result, lengths):
    B, S, D = v_cache.shape
    ws, need = workspace_for(B, S, D, v_cache.device)
    _check(load_library().mli_softmax_v(_p(softmax_result), _p(v_cache), _p(lengths), _p(attention_result), B, S, D,
                                        _p(ws), need, _stream()), "mli_softmax_v")


def inference_self_attention(inp_embedding, lengths, wk, wq, wv, new_batch_idx, kt_cache, v_cache, q_output,
                             qkt_output, attention_result, n_new_items):
    B, S, Din = inp_embedding.shape
    Dout = wk.shape[1]
    ws, need = workspace_for(B, S, Dout, inp_embedding.device)
    _check(load_library().mli_inference_self_attention(
        _p(inp_embedding), _p(lengths), _p(wk), _p(wq), _p(wv), _p(new_batch_idx), _p(kt_cache), _p(v_cache),
        _p(q_output), _p(qkt_output), _p(attention_result), B, S, Din, Dout, n_new_items, _p(ws), need, _stream()),
        "mli_inference_self_attention")


def self_attention_lean(inp_embedding, lengths, wk, wq, wv, new_batch_idx, kt_cache, v_cache, q_output, attention_result,
                        n_new_items):
    """What SelfAttentionLayer runs: the contiguous composition without the qkt_output scratch (mli_self_attention_lean)."""
    B, S, Din = inp_embedding.shape
    Dout = wk.shape[1]
    ws, need = workspace_for(B, S, Dout, inp_embedding.device)
    _check(load_library().mli_self_attention_lean(
        _p(inp_embedding), _p(lengths), _p(wk), _p(wq), _p(wv), _p(new_batch_idx), _p(kt_cache), _p(v_cache),
        _p(q_output), _p(attention_result), B, S, Din, Dout, n_new_items, _p(ws), need, _stream()),
        "mli_self_attention_lean")


def decode_scan_contiguous(q_output, kt_cache, v_cache, lengths, attention_result):
    """The single-launch scan of the lean contiguous composition on its own (mli_decode_scan_contiguous)."""
    B, D, S = kt_cache.shape
    ws, need = workspace_for(B, S, D, q_output.device)
    _check(load_library().mli_decode_scan_contiguous(_p(q_output), _p(kt_cache), _p(v_cache), _p(lengths),
                                                     _p(attention_result), B, S, D, _p(ws), need, _stream()),
           "mli_decode_scan_contiguous")


# ---- paged path (page_table: int64 [B, S/16] tensor of device addresses) -----------------------
def launch_fill_new_k_v_cache_paged_attention(page_table, new_batch_idx, lengths, wk, wv, n_new_items, n_sequence):
    B = page_table.shape[0]
    _check(load_library().mli_fill_new_k_v_cache_paged(_p(page_table), _p(new_batch_idx), _p(lengths), _p(wk), _p(wv),
                                                       B, n_sequence, wk.shape[0], n_new_items, _stream()),
           "mli_fill_new_k_v_cache_paged")


# the reference's warp-tiled variant is the same MFMA kernel here
launch_fill_new_k_v_cache_paged_attention_warp_tiling = launch_fill_new_k_v_cache_paged_attention


def launch_get_latest_k_q_v_paged_attention(page_table, lengths, wk, wq, wv, q_output, n_sequence):
    B = page_table.shape[0]
    _check(load_library().mli_get_latest_k_q_v_paged(_p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv),
                                                     _p(q_output), B, n_sequence, wq.shape[0], _stream()),
           "mli_get_latest_k_q_v_paged")


def launch_qkt_paged_attention(q_output, page_table, lengths, qkt_output):
    B, D = q_output.shape
    _check(load_library().mli_qkt_paged(_p(q_output), _p(page_table), _p(lengths), _p(qkt_output), B,
                                        qkt_output.shape[1], D, _stream()), "mli_qkt_paged")


def launch_softmax_v_paged_attention(softmax_result, page_table, attention_result, lengths):
    B, S = softmax_result.shape
    D = attention_result.shape[1]
    ws, need = workspace_for(B, S, D, softmax_result.device)
    _check(load_library().mli_softmax_v_paged(_p(softmax_result), _p(page_table), _p(lengths), _p(attention_result),
                                              B, S, D, _p(ws), need, _stream()), "mli_softmax_v_paged")


def paged_attention(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, qkt_output, attention_result,
                    n_new_items, n_sequence):
    B = page_table.shape[0]
    D = wk.shape[0]
    ws, need = workspace_for(B, n_sequence, D, q_output.device)
    _check(load_library().mli_paged_attention(_p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv), _p(new_batch_idx),
                                              _p(q_output), _p(qkt_output), _p(attention_result), B, n_sequence, D,
                                              n_new_items, _p(ws), need, _stream()), "mli_paged_attention")


class GemmHandle:
    """Stands where the reference passes a cublasHandle_t (include/kernels/paged_attention.h:46-63); empty."""


def launch_get_latest_k_q_v_paged_attention_cublas(page_table, lengths, latest_emb, wk, wq, wv, q_output,
                                                   temp_placeholder, handle, n_sequence):
    """The reference's argument list (paged_attention.h:57-63).  latest_emb / temp_placeholder were scratch of the
    three cublasSgemm calls: accepted, never touched (one gather-GEMM-scatter kernel needs neither)."""
    assert isinstance(handle, GemmHandle) and latest_emb.shape == q_output.shape == temp_placeholder.shape
    launch_get_latest_k_q_v_paged_attention(page_table, lengths, wk, wq, wv, q_output, n_sequence)


def paged_attention_with_cublas(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, qkt_output, attention_result,
                                latest_emb=None, temp_placeholder=None, n_new_items=None, n_sequence=None, handle=None):
    """paged_attention.h:46-54 (…, latest_emb, temp_placeholder, n_new_items, n_sequence, handle); the short form
    (…, attention_result, n_new_items, n_sequence) of paged_attention is accepted too."""
    if n_sequence is None:  # called with paged_attention's positional list
        latest_emb, temp_placeholder, n_new_items, n_sequence = None, None, latest_emb, temp_placeholder
    else:
        assert isinstance(handle, GemmHandle) and latest_emb.shape == q_output.shape == temp_placeholder.shape
    paged_attention(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, qkt_output, attention_result,
                    n_new_items, n_sequence)


# ---- bf16 paged path (extension; BASELINE config 4).  page_table addresses point at bf16 pages ----------
def launch_fill_new_k_v_cache_paged_attention_bf16(page_table, new_batch_idx, lengths, wk, wv, n_new_items, n_sequence):
    B = page_table.shape[0]
    _check(load_library().mli_fill_new_k_v_cache_paged_bf16(_p(page_table), _p(new_batch_idx), _p(lengths), _p(wk),
                                                            _p(wv), B, n_sequence, wk.shape[0], n_new_items,
                                                            _stream()), "mli_fill_new_k_v_cache_paged_bf16")


def launch_get_latest_k_q_v_paged_attention_bf16(page_table, lengths, wk, wq, wv, q_output, n_sequence):
    B = page_table.shape[0]
    _check(load_library().mli_get_latest_k_q_v_paged_bf16(_p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv),
                                                          _p(q_output), B, n_sequence, wq.shape[0], _stream()),
           "mli_get_latest_k_q_v_paged_bf16")


def launch_qkt_paged_attention_bf16(q_output, page_table, lengths, qkt_output):
    B, D = q_output.shape
    _check(load_library().mli_qkt_paged_bf16(_p(q_output), _p(page_table), _p(lengths), _p(qkt_output), B,
                                             qkt_output.shape[1], D, _stream()), "mli_qkt_paged_bf16")


def launch_softmax_v_paged_attention_bf16(softmax_result, page_table, attention_result, lengths):
    B, S = softmax_result.shape
    D = attention_result.shape[1]
    ws, need = workspace_for(B, S, D, softmax_result.device)
    _check(load_library().mli_softmax_v_paged_bf16(_p(softmax_result), _p(page_table), _p(lengths),
                                                   _p(attention_result), B, S, D, _p(ws), need, _stream()),
           "mli_softmax_v_paged_bf16")


def paged_attention_bf16(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, qkt_output, attention_result,
                         n_new_items, n_sequence):
    B = page_table.shape[0]
    D = wk.shape[0]
    ws, need = workspace_for(B, n_sequence, D, q_output.device)
    _check(load_library().mli_paged_attention_bf16(_p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv),
                                                   _p(new_batch_idx), _p(q_output), _p(qkt_output),
                                                   _p(attention_result), B, n_sequence, D, n_new_items, _p(ws), need,
                                                   _stream()), "mli_paged_attention_bf16")


def launch_paged_attention_encoder_kernel_bf16(emb_table, wpe, inp, page_table, lengths, new_item_indices, n_new_items):
    B, S = inp.shape
    _check(load_library().mli_paged_attention_encoder_bf16(_p(emb_table), _p(wpe), _p(inp), _p(page_table),
                                                           _p(lengths), _p(new_item_indices), B, S,
                                                           emb_table.shape[1], n_new_items, _stream()),
           "mli_paged_attention_encoder_bf16")


def launch_paged_attention_decoder_multi_rounds_bf16(batch_result, emb_table, emb_score, wpe_table, page_table,
                                                     lengths, decoder_result, i_decoder):
    B, D = batch_result.shape
    n_res = decoder_result.shape[1] if decoder_result.dim() == 2 else 1
    _check(load_library().mli_paged_decoder_multi_rounds_bf16(_p(batch_result), _p(emb_table), _p(emb_score),
                                                              _p(wpe_table), _p(page_table), _p(lengths),
                                                              _p(decoder_result), B, emb_table.shape[0],
                                                              wpe_table.shape[0], D, n_res, i_decoder, _stream()),
           "mli_paged_decoder_multi_rounds_bf16")


def decode_scan_paged(q_output, page_table, lengths, qkt_output, attention_result, elem_bf16, phases=3, n_sequence=None):
    """Single-pass scores + masked softmax + softmax.V over the pages (mli_decode_scan_paged).  phases & 4 = lean mode:
    qkt_output may be None (pass n_sequence then)."""
    B, D = q_output.shape
    S = qkt_output.shape[1] if qkt_output is not None else n_sequence
    ws, need = workspace_for(B, S, D, q_output.device)
    _check(load_library().mli_decode_scan_paged(_p(q_output), _p(page_table), _p(lengths), _p(qkt_output),
                                                _p(attention_result), B, S, D, int(elem_bf16), int(phases), _p(ws),
                                                need, _stream()), "mli_decode_scan_paged")


def _elem_of(wk, elem):
    """MLI_ELEM_* of the pages: given, or from the weights' dtype (fp8 pages come with bf16 weights: say so)."""
    return int(wk.dtype == torch.bfloat16) if elem is None else int(elem)


def _lean_call(name, front, B, n_sequence, D, extra, n_heads, elem, device):
    """One lean entry point: the workspace for n_heads heads, then name(*front, B, n_sequence, D, *extra, elem, workspace)."""
    ws, need = workspace_for(B, n_sequence, D, device, n_heads)
    _check(getattr(load_library(), name)(*map(_p, front), B, n_sequence, D, *map(int, extra), int(elem), _p(ws), need,
                                         _stream()), name)


def decode_scan_paged_heads(q_output, page_table, lengths, attention_result, n_heads, elem, n_sequence):
    """The multi-head single-pass scan (mli_decode_scan_paged_heads): head h owns columns [h * D / n_heads, ...) of q, K and V,
    one softmax per head; lean form.  n_heads = 1 is decode_scan_paged(phases=7)."""
    B, D = q_output.shape
    _lean_call("mli_decode_scan_paged_heads", (q_output, page_table, lengths, attention_result), B, n_sequence, D, (n_heads,),
               n_heads, elem, q_output.device)


def decode_scan_paged_window(q_output, page_table, lengths, attention_result, n_heads, window, elem, n_sequence):
    """The sliding-window scan (mli_decode_scan_paged_window): row b attends slots [max(0, L - window), L) only; lean
    form, n_heads heads.  window >= n_sequence is decode_scan_paged(phases=7) / decode_scan_paged_heads."""
    B, D = q_output.shape
    _lean_call("mli_decode_scan_paged_window", (q_output, page_table, lengths, attention_result), B, n_sequence, D,
               (n_heads, window), n_heads, elem, q_output.device)


def decode_scan_paged_sinks(q_output, page_table, lengths, attention_result, n_heads, window, sinks, elem, n_sequence):
    """The sliding-window scan with attention sinks (mli_decode_scan_paged_sinks): row b attends its first `sinks` slots and
    slots [max(0, L - window), L); lean form, n_heads heads.  sinks = 0 is decode_scan_paged_window; sinks + window >=
    n_sequence is decode_scan_paged(phases=7) / decode_scan_paged_heads."""
    B, D = q_output.shape
    _lean_call("mli_decode_scan_paged_sinks", (q_output, page_table, lengths, attention_result), B, n_sequence, D,
               (n_heads, window, sinks), n_heads, elem, q_output.device)


def decode_scan_paged_gqa(q_output, page_table, lengths, attention_result, n_heads, n_kv_heads, window, sinks, elem, n_sequence):
    """The multi-head scan with grouped-query attention (mli_decode_scan_paged_gqa): query head h attends K/V head
    h // (n_heads // n_kv_heads), whose columns are [that * D / n_heads, ...) of the K and V segments; the columns beyond
    n_kv_heads * D / n_heads are never read.  window <= 0 (or None): no window; sinks 0 (or None): none.  n_kv_heads ==
    n_heads is decode_scan_paged_sinks."""
    B, D = q_output.shape
    _lean_call("mli_decode_scan_paged_gqa", (q_output, page_table, lengths, attention_result), B, n_sequence, D,
               (n_heads, n_kv_heads, window or 0, sinks or 0), n_heads, elem, q_output.device)


def alibi_slopes(n_heads):
    """The standard ALiBi slopes of n_heads heads (mli_alibi_slopes): a float32 numpy array; 2^(-8 (i + 1) / n) over the
    largest power of two n <= n_heads, then every other slope of the 2 n series."""
    out = np.empty(max(int(n_heads), 0), np.float32)
    _check(load_library().mli_alibi_slopes(int(n_heads), out.ctypes.data_as(ctypes.c_void_p)), "mli_alibi_slopes")
    return out


def rope_table(n_sequence, head_dim, theta=10000.0):
    """The standard rotary table (mli_rope_table): a float32 numpy array [n_sequence, head_dim // 2, 2] of (cos, sin) of
    s * theta^(-2 i / head_dim), computed in double.  Copy it to the device for the rope= arguments."""
    out = np.empty((max(int(n_sequence), 0), max(int(head_dim), 0) // 2, 2), np.float32)
    _check(load_library().mli_rope_table(int(n_sequence), int(head_dim), float(theta), out.ctypes.data_as(ctypes.c_void_p)),
           "mli_rope_table")
    return out


def decode_scan_paged_alibi(q_output, page_table, lengths, attention_result, n_heads, n_kv_heads, window, sinks, slopes, elem,
                            n_sequence):
    """decode_scan_paged_gqa with ALiBi (mli_decode_scan_paged_alibi): slopes[h] * (s - (L - 1)) is added to query head h's
    scaled score of the row's absolute slot s.  slopes: n_heads float32 values on the device; n_heads >= 2; n_kv_heads None
    or n_heads: no grouping."""
    B, D = q_output.shape
    ws, need = workspace_for(B, n_sequence, D, q_output.device, n_heads)
    _check(load_library().mli_decode_scan_paged_alibi(_p(q_output), _p(page_table), _p(lengths), _p(attention_result), B,
                                                      int(n_sequence), D, int(n_heads), int(n_kv_heads or n_heads),
                                                      int(window or 0), int(sinks or 0), _p(slopes), int(elem), _p(ws), need,
                                                      _stream()), "mli_decode_scan_paged_alibi")


def decode_scan_paged_softcap(q_output, page_table, lengths, attention_result, n_heads, n_kv_heads, window, sinks, softcap, elem,
                              n_sequence):
    """decode_scan_paged_gqa with logit soft-capping (mli_decode_scan_paged_softcap): query head h's scaled score x of an
    attended slot becomes softcap * tanh(x / softcap).  softcap: a finite float > 0; n_heads >= 2; n_kv_heads None or n_heads:
    no grouping."""
    B, D = q_output.shape
    ws, need = workspace_for(B, n_sequence, D, q_output.device, n_heads)
    _check(load_library().mli_decode_scan_paged_softcap(_p(q_output), _p(page_table), _p(lengths), _p(attention_result), B,
                                                        int(n_sequence), D, int(n_heads), int(n_kv_heads or n_heads),
                                                        int(window or 0), int(sinks or 0), float(softcap), int(elem), _p(ws),
                                                        need, _stream()), "mli_decode_scan_paged_softcap")


def _sink_logits_alone(alibi_slopes, softcap):
    if alibi_slopes is not None:
        raise ValueError("attention-sink logits and ALiBi are not combined")
    if softcap is not None:
        raise ValueError("attention-sink logits and logit soft-capping are not combined")


def decode_scan_paged_sink_logits(q_output, page_table, lengths, attention_result, n_heads, n_kv_heads, window, sinks, sink_logits,
                                  elem, n_sequence):
    """decode_scan_paged_gqa with a learned attention-sink logit per query head (mli_decode_scan_paged_sink_logits):
    sink_logits[h] takes part in head h's softmax as one more logit without a value row -- it enters the maximum and the
    denominator, once per (row, head).  sink_logits: n_heads float32 values on the device, each finite or -inf (-inf: no sink);
    n_heads >= 2; n_kv_heads None or n_heads: no grouping.  `sinks` is the count of sink TOKENS, another switch."""
    B, D = q_output.shape
    ws, need = workspace_for(B, n_sequence, D, q_output.device, n_heads)
    _check(load_library().mli_decode_scan_paged_sink_logits(_p(q_output), _p(page_table), _p(lengths), _p(attention_result), B,
                                                            int(n_sequence), D, int(n_heads), int(n_kv_heads or n_heads),
                                                            int(window or 0), int(sinks or 0), _p(sink_logits), int(elem), _p(ws),
                                                            need, _stream()), "mli_decode_scan_paged_sink_logits")


def paged_attention_lean(page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result, n_new_items,
                         n_sequence, elem=None, n_heads=1, window=None, sinks=None, n_kv_heads=None, alibi_slopes=None,
                         rope=None, softcap=None, sink_logits=None):
    """What the attention layers run: the paged composition without materialising scores / probabilities
    (mli_paged_attention_lean); page element type = elem (ELEM_*), default from the weights' dtype.  n_heads != 1: the
    multi-head form (mli_paged_attention_lean_heads); window given: the sliding-window form
    (mli_paged_attention_lean_window); sinks given as well: the first `sinks` tokens of every row stay attended
    (mli_paged_attention_lean_sinks); n_kv_heads given: grouped-query attention with that many K/V heads
    (mli_paged_attention_lean_gqa; wk / wv keep their [D, D] shape, their first n_kv_heads * D / n_heads columns matter);
    alibi_slopes given (n_heads float32 values on the device): the scan adds the position bias of decode_scan_paged_alibi
    (mli_paged_attention_lean_alibi), with any of window, sinks and n_kv_heads;
    rope given (a [n_sequence, D / n_heads / 2, 2] float32 (cos, sin) table on the device): fill and projection rotate K and q
    by the token's absolute slot (mli_paged_attention_lean_rope), with any of the above;
    softcap given (a finite float > 0): the scan caps its scaled scores as decode_scan_paged_softcap does
    (mli_paged_attention_lean_softcap), with any of window, sinks, n_kv_heads and rope, never with alibi_slopes;
    sink_logits given (n_heads float32 values on the device): the scan counts a learned sink logit per query head as
    decode_scan_paged_sink_logits does (mli_paged_attention_lean_sink_logits), with any of window, sinks, n_kv_heads and rope,
    never with alibi_slopes or softcap."""
    if sink_logits is not None:
        _sink_logits_alone(alibi_slopes, softcap)
        if sinks is not None and window is None:
            raise ValueError("sinks exist beside a window: pass window= as well")
        B, D = page_table.shape[0], wk.shape[0]
        ws, need = workspace_for(B, n_sequence, D, q_output.device, n_heads)
        _check(load_library().mli_paged_attention_lean_sink_logits(
            _p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv), _p(new_batch_idx), _p(q_output), _p(attention_result), B,
            int(n_sequence), D, int(n_new_items), int(n_heads), int(n_kv_heads or n_heads), int(window or 0), int(sinks or 0),
            _p(sink_logits), _p(rope), _elem_of(wk, elem), _p(ws), need, _stream()), "mli_paged_attention_lean_sink_logits")
        return
    if softcap is not None:
        if alibi_slopes is not None:
            raise ValueError("logit soft-capping and ALiBi are not combined")
        if sinks is not None and window is None:
            raise ValueError("sinks exist beside a window: pass window= as well")
        B, D = page_table.shape[0], wk.shape[0]
        ws, need = workspace_for(B, n_sequence, D, q_output.device, n_heads)
        _check(load_library().mli_paged_attention_lean_softcap(
            _p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv), _p(new_batch_idx), _p(q_output), _p(attention_result), B,
            int(n_sequence), D, int(n_new_items), int(n_heads), int(n_kv_heads or n_heads), int(window or 0), int(sinks or 0),
            float(softcap), _p(rope), _elem_of(wk, elem), _p(ws), need, _stream()), "mli_paged_attention_lean_softcap")
        return
    if rope is not None:
        if sinks is not None and window is None:
            raise ValueError("sinks exist beside a window: pass window= as well")
        B, D = page_table.shape[0], wk.shape[0]
        ws, need = workspace_for(B, n_sequence, D, q_output.device, n_heads)
        _check(load_library().mli_paged_attention_lean_rope(
            _p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv), _p(new_batch_idx), _p(q_output), _p(attention_result), B,
            int(n_sequence), D, int(n_new_items), int(n_heads), int(n_kv_heads or n_heads), int(window or 0), int(sinks or 0),
            _p(alibi_slopes), _p(rope), _elem_of(wk, elem), _p(ws), need, _stream()), "mli_paged_attention_lean_rope")
        return
    if alibi_slopes is not None:
        if sinks is not None and window is None:
            raise ValueError("sinks exist beside a window: pass window= as well")
        B, D = page_table.shape[0], wk.shape[0]
        ws, need = workspace_for(B, n_sequence, D, q_output.device, n_heads)
        _check(load_library().mli_paged_attention_lean_alibi(
            _p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv), _p(new_batch_idx), _p(q_output), _p(attention_result), B,
            int(n_sequence), D, int(n_new_items), int(n_heads), int(n_kv_heads or n_heads), int(window or 0), int(sinks or 0),
            _p(alibi_slopes), _elem_of(wk, elem), _p(ws), need, _stream()), "mli_paged_attention_lean_alibi")
        return
    if n_kv_heads is not None:
        if sinks is not None and window is None:
            raise ValueError("sinks exist beside a window: pass window= as well")
        name, extra = "mli_paged_attention_lean_gqa", (n_new_items, n_heads, n_kv_heads, window or 0, sinks or 0)
    elif sinks is not None:
        if window is None:
            raise ValueError("sinks exist beside a window: pass window= as well")
        name, extra = "mli_paged_attention_lean_sinks", (n_new_items, n_heads, window, sinks)
    elif window is not None:
        name, extra = "mli_paged_attention_lean_window", (n_new_items, n_heads, window)
    elif n_heads != 1:
        name, extra = "mli_paged_attention_lean_heads", (n_new_items, n_heads)
    else:
        name, extra = "mli_paged_attention_lean", (n_new_items,)
    _lean_call(name, (page_table, lengths, wk, wq, wv, new_batch_idx, q_output, attention_result), page_table.shape[0],
               n_sequence, wk.shape[0], extra, n_heads, _elem_of(wk, elem), q_output.device)


def paged_prefill(emb_table, wpe, inp, page_table, lengths, new_item_indices, wk, wv, n_new_items, elem=None, window=None,
                  sinks=None, n_heads=1, rope=None):
    """Encoder + prefill fill in one launch (mli_paged_prefill); page element type = elem, default from the weights.
    window given (sinks beside it): the prefill of the rows' live tokens (mli_paged_prefill_window) -- pages between the
    sink pages and the window's first page are neither looked up nor written.
    rope given (a [S, D / n_heads / 2, 2] float32 (cos, sin) table on the device): K is stored rotated by the token's slot
    (mli_paged_prefill_rope), with or without a window."""
    B, S = inp.shape
    if sinks is not None and window is None:
        raise ValueError("sinks exist beside a window: pass window= as well")
    if rope is not None:
        _check(load_library().mli_paged_prefill_rope(_p(emb_table), _p(wpe), _p(inp), _p(page_table), _p(lengths),
                                                     _p(new_item_indices), _p(wk), _p(wv), B, S, emb_table.shape[1],
                                                     n_new_items, window or 0, sinks or 0, int(n_heads), _p(rope),
                                                     _elem_of(wk, elem), _stream()), "mli_paged_prefill_rope")
        return
    if window is not None:
        _check(load_library().mli_paged_prefill_window(_p(emb_table), _p(wpe), _p(inp), _p(page_table), _p(lengths),
                                                       _p(new_item_indices), _p(wk), _p(wv), B, S, emb_table.shape[1],
                                                       n_new_items, window, sinks or 0, _elem_of(wk, elem), _stream()),
               "mli_paged_prefill_window")
        return
    _check(load_library().mli_paged_prefill(_p(emb_table), _p(wpe), _p(inp), _p(page_table), _p(lengths),
                                            _p(new_item_indices), _p(wk), _p(wv), B, S, emb_table.shape[1], n_new_items,
                                            _elem_of(wk, elem), _stream()), "mli_paged_prefill")


def prefill(emb_table, wpe, inp, inp_embedding, lengths, new_item_indices, wk, wv, kt_cache, v_cache, n_new_items):
    """Encoder + prefill fill in one launch, contiguous layout (mli_prefill)."""
    B, S, Din = inp_embedding.shape
    _check(load_library().mli_prefill(_p(emb_table), _p(wpe), _p(inp), _p(inp_embedding), _p(lengths),
                                      _p(new_item_indices), _p(wk), _p(wv), _p(kt_cache), _p(v_cache), B, S, Din,
                                      wk.shape[1], n_new_items, _stream()), "mli_prefill")


_decoder_scratch = {}


def decoder_scratch_for(n_batch, n_vocab, device):
    lib = load_library()
    need = int(lib.mli_decoder_scratch_bytes(n_batch, n_vocab))
    index = device.index if device.index is not None else torch.cuda.current_device()
    key = (index, torch.cuda.current_stream(index).cuda_stream)
    buf = _decoder_scratch.get(key)
    if buf is None or buf.numel() < need:
        buf = torch.zeros(max(need, 16), dtype=torch.uint8, device=device)
        _decoder_scratch[key] = buf
    return buf, need


def decoder_fused(batch_result, emb_table, wpe_table, inp_embedding, lengths, decoder_result):
    """launch_decoder with the argmax as the logits GEMM's epilogue (no emb_score)."""
    B, D = batch_result.shape
    sc, need = decoder_scratch_for(B, emb_table.shape[0], batch_result.device)
    _check(load_library().mli_decoder_fused(_p(batch_result), _p(emb_table), _p(wpe_table), _p(inp_embedding),
                                            _p(lengths), _p(decoder_result), B, emb_table.shape[0], wpe_table.shape[0],
                                            D, _p(sc), need, _stream()), "mli_decoder_fused")


def paged_decoder_fused(batch_result, emb_table, wpe_table, page_table, lengths, decoder_result, i_decoder, elem_bf16):
    """launch_paged_attention[_cublas]_decoder_multi_rounds with the argmax as the logits GEMM's epilogue."""
    B, D = batch_result.shape
    n_res = decoder_result.shape[1] if decoder_result.dim() == 2 else 1
    sc, need = decoder_scratch_for(B, emb_table.shape[0], batch_result.device)
    _check(load_library().mli_paged_decoder_fused(_p(batch_result), _p(emb_table), _p(wpe_table), _p(page_table),
                                                  _p(lengths), _p(decoder_result), B, emb_table.shape[0],
                                                  wpe_table.shape[0], D, n_res, i_decoder, int(elem_bf16), _p(sc), need,
                                                  _stream()), "mli_paged_decoder_fused")


def _sampling_args(temperature, top_k, top_p, seed):
    """The four per-row parameter arrays of the sampled heads (device tensors: f32, i32, f32, i64)."""
    for t, dt, name in ((temperature, torch.float32, "temperature"), (top_k, torch.int32, "top_k"),
                        (top_p, torch.float32, "top_p"), (seed, torch.int64, "seed")):
        if t.dtype != dt:
            raise MliError(f"{name} must be {dt}, got {t.dtype}")
    return _p(temperature), _p(top_k), _p(top_p), _p(seed)


def sample_tokens(logits, temperature, top_k, top_p, seed, lengths, tokens=None):
    """EXTENSION: seeded temperature / top-k / top-p draw per row of logits [B, V] at position lengths[b]
    (mli_sample_tokens).  Returns tokens [B] int32."""
    B, V = logits.shape
    if tokens is None:
        tokens = torch.empty(B, dtype=torch.int32, device=logits.device)
    lib = load_library()
    need = int(lib.mli_sample_scratch_bytes(B, V))
    sc = torch.empty(max(need, 16), dtype=torch.uint8, device=logits.device) if need else None
    _check(lib.mli_sample_tokens(_p(logits), *_sampling_args(temperature, top_k, top_p, seed), _p(lengths), _p(tokens),
                                 B, V, _p(sc), need, _stream()), "mli_sample_tokens")
    return tokens


def sample_tokens_logprobs(logits, temperature, top_k, top_p, seed, lengths, n_top=0, tokens=None):
    """EXTENSION: sample_tokens plus, per row, the natural-log probability of the emitted token under the raw distribution of
    the row's finite logits and the n_top (0 .. 8) candidates of largest logit with theirs (mli_sample_tokens_logprobs;
    DESIGN 3.6c).  Returns (tokens [B] int32, token_logprob [B] float32, top_ids [B, n_top] int32, top_logprobs [B, n_top]
    float32)."""
    lib = load_library()
    B, V = logits.shape
    n_top = int(n_top)
    if tokens is None:
        tokens = torch.empty(B, dtype=torch.int32, device=logits.device)
    token_logprob = torch.empty(B, dtype=torch.float32, device=logits.device)
    top_ids = torch.empty((B, max(n_top, 0)), dtype=torch.int32, device=logits.device)
    top_logprobs = torch.empty((B, max(n_top, 0)), dtype=torch.float32, device=logits.device)
    need = int(lib.mli_sample_scratch_bytes(B, V))
    sc = torch.empty(max(need, 16), dtype=torch.uint8, device=logits.device) if need else None
    _check(lib.mli_sample_tokens_logprobs(_p(logits), *_sampling_args(temperature, top_k, top_p, seed), _p(lengths), _p(tokens),
                                          _p(token_logprob), _p(top_ids) if n_top > 0 else None,
                                          _p(top_logprobs) if n_top > 0 else None, B, V, n_top, _p(sc), need, _stream()),
           "mli_sample_tokens_logprobs")
    return tokens, token_logprob, top_ids, top_logprobs


def _segments(segments, device):
    """The four device arrays of a list of segments [(row, first position, count)] with dense offsets in list order, the
    largest count and the number of positions."""
    rows = [int(r) for r, _, _ in segments]
    first = [int(f) for _, f, _ in segments]
    count = [int(n) for _, _, n in segments]
    offset = [sum(count[:i]) for i in range(len(count))]
    arrays = [torch.tensor(a, dtype=torch.int32, device=device) for a in (rows, first, count, offset)]
    return arrays, max(count, default=0), sum(count)


def prompt_scan_tq(emb_dim, n_heads, elem):
    """The consecutive query positions a workgroup of prompt_scan_paged shares its K / V loads among (mli_prompt_scan_tq)."""
    tq = int(load_library().mli_prompt_scan_tq(int(emb_dim), int(n_heads), int(elem)))
    if tq < 0:
        raise MliError(f"Hip Failure: mli_prompt_scan_tq returned {tq}")
    return tq


def prompt_scan_paged(q, page_table, segments, out, n_batch, n_sequence, elem, n_heads=1, n_kv_heads=None, window=None,
                      sinks=None, seg_arrays=None, softcap=None, sink_logits=None):
    """EXTENSION: the causal multi-query paged scan (mli_prompt_scan_paged).  segments = [(row, first position,
    count)]: query j of a segment is position first + j of its row and attends the slots s <= its position (inside the window or
    among the sinks); q and out [n_q, D] hold the queries in list order.  seg_arrays = (rows, first, count, offset, max_count)
    device arrays replace the list.  softcap given (a finite float > 0, n_heads >= 2): every scaled score x becomes
    softcap * tanh(x / softcap) (mli_prompt_scan_paged_softcap).  sink_logits given (n_heads float32 values on the device,
    n_heads >= 2; never with softcap): query t gets what decode_scan_paged_sink_logits gives a row of length t + 1
    (mli_prompt_scan_paged_sink_logits)."""
    if sink_logits is not None:
        _sink_logits_alone(None, softcap)
    n_q, D = q.shape
    if seg_arrays is None:
        arrays, max_count, _ = _segments(segments, q.device)
    else:
        arrays, max_count = list(seg_arrays[:4]), int(seg_arrays[4])
    if sink_logits is not None:
        _check(load_library().mli_prompt_scan_paged_sink_logits(_p(q), _p(page_table), *map(_p, arrays), _p(out),
                                                                int(arrays[0].numel()), max_count, n_q, int(n_batch),
                                                                int(n_sequence), D, int(n_heads), int(n_kv_heads or n_heads),
                                                                int(window or 0), int(sinks or 0), _p(sink_logits), int(elem),
                                                                _stream()), "mli_prompt_scan_paged_sink_logits")
        return out
    if softcap is not None:
        _check(load_library().mli_prompt_scan_paged_softcap(_p(q), _p(page_table), *map(_p, arrays), _p(out),
                                                            int(arrays[0].numel()), max_count, n_q, int(n_batch), int(n_sequence),
                                                            D, int(n_heads), int(n_kv_heads or n_heads), int(window or 0),
                                                            int(sinks or 0), float(softcap), int(elem), _stream()),
               "mli_prompt_scan_paged_softcap")
        return out
    _check(load_library().mli_prompt_scan_paged(_p(q), _p(page_table), *map(_p, arrays), _p(out), int(arrays[0].numel()),
                                                max_count, n_q, int(n_batch), int(n_sequence), D, int(n_heads),
                                                int(n_kv_heads or n_heads), int(window or 0), int(sinks or 0), int(elem),
                                                _stream()), "mli_prompt_scan_paged")
    return out


def prompt_project_q(page_table, segments, wq, n_batch, n_sequence, elem):
    """q [n_q, D] float32 = x(row, position) . wq for the positions of the segments (mli_prompt_project_q)."""
    D = wq.shape[0]
    arrays, max_count, n_q = _segments(segments, wq.device)
    gathered = torch.empty(max(n_q, 1) * D, dtype=torch.float32, device=wq.device)
    q = torch.empty((n_q, D), dtype=torch.float32, device=wq.device)
    _check(load_library().mli_prompt_project_q(_p(page_table), *map(_p, arrays), _p(wq), _p(gathered), _p(q), len(segments),
                                               max_count, n_q, int(n_batch), int(n_sequence), D, int(elem), _stream()),
           "mli_prompt_project_q")
    return q


def _score_outputs(n, n_top, device):
    return (torch.empty(n, dtype=torch.float32, device=device), torch.empty((n, max(n_top, 0)), dtype=torch.int32, device=device),
            torch.empty((n, max(n_top, 0)), dtype=torch.float32, device=device))


def score_tokens_logprobs(logits, targets, n_top=0):
    """EXTENSION: the figures of sample_tokens_logprobs for the token targets[i] each row is GIVEN (mli_score_tokens_logprobs).
    Returns (token_logprob [n], top_ids [n, n_top], top_logprobs [n, n_top])."""
    n, V = logits.shape
    n_top = int(n_top)
    if targets.dtype != torch.int32:
        raise MliError(f"targets must be int32, got {targets.dtype}")
    token_logprob, top_ids, top_logprobs = _score_outputs(n, n_top, logits.device)
    _check(load_library().mli_score_tokens_logprobs(_p(logits), _p(targets), _p(token_logprob),
                                                    _p(top_ids) if n_top > 0 else None,
                                                    _p(top_logprobs) if n_top > 0 else None, n, V, n_top, _stream()),
           "mli_score_tokens_logprobs")
    return token_logprob, top_ids, top_logprobs


def paged_prompt_logprobs(page_table, inp, wq, emb_table, segments, n_batch, n_sequence, elem, n_top=0, n_heads=1,
                          n_kv_heads=None, window=None, sinks=None, softcap=None, sink_logits=None):
    """EXTENSION: prompt log-probabilities for the positions of the segments from the pages a prefill has written
    (mli_paged_prompt_logprobs): projection, causal scan, logits, scoring of inp[row, position + 1].  Returns (token_logprob
    [n], top_ids [n, n_top], top_logprobs [n, n_top]) in list order.  softcap given: the scan with logit soft-capping
    (mli_paged_prompt_logprobs_softcap).  sink_logits given (never with softcap): the scan with a learned sink logit per query
    head (mli_paged_prompt_logprobs_sink_logits)."""
    if sink_logits is not None:
        _sink_logits_alone(None, softcap)
    lib = load_library()
    D, V = wq.shape[0], emb_table.shape[0]
    n_top = int(n_top)
    arrays, max_count, n = _segments(segments, wq.device)
    token_logprob, top_ids, top_logprobs = _score_outputs(n, n_top, wq.device)
    need = int(lib.mli_prompt_logprobs_scratch_bytes(n, D, V))
    sc = torch.empty(max(need, 16), dtype=torch.uint8, device=wq.device)
    if sink_logits is not None:
        _check(lib.mli_paged_prompt_logprobs_sink_logits(
            _p(page_table), _p(inp), _p(wq), _p(emb_table), *map(_p, arrays), _p(token_logprob),
            _p(top_ids) if n_top > 0 else None, _p(top_logprobs) if n_top > 0 else None, len(segments), max_count, n,
            int(n_batch), int(n_sequence), D, V, int(n_heads), int(n_kv_heads or n_heads), int(window or 0), int(sinks or 0),
            _p(sink_logits), int(elem), n_top, _p(sc), need, _stream()), "mli_paged_prompt_logprobs_sink_logits")
        return token_logprob, top_ids, top_logprobs
    if softcap is not None:
        _check(lib.mli_paged_prompt_logprobs_softcap(
            _p(page_table), _p(inp), _p(wq), _p(emb_table), *map(_p, arrays), _p(token_logprob),
            _p(top_ids) if n_top > 0 else None, _p(top_logprobs) if n_top > 0 else None, len(segments), max_count, n,
            int(n_batch), int(n_sequence), D, V, int(n_heads), int(n_kv_heads or n_heads), int(window or 0), int(sinks or 0),
            float(softcap), int(elem), n_top, _p(sc), need, _stream()), "mli_paged_prompt_logprobs_softcap")
        return token_logprob, top_ids, top_logprobs
    _check(lib.mli_paged_prompt_logprobs(_p(page_table), _p(inp), _p(wq), _p(emb_table), *map(_p, arrays), _p(token_logprob),
                                         _p(top_ids) if n_top > 0 else None, _p(top_logprobs) if n_top > 0 else None,
                                         len(segments), max_count, n, int(n_batch), int(n_sequence), D, V, int(n_heads),
                                         int(n_kv_heads or n_heads), int(window or 0), int(sinks or 0), int(elem), n_top,
                                         _p(sc), need, _stream()), "mli_paged_prompt_logprobs")
    return token_logprob, top_ids, top_logprobs


def _sampled_scratch(n_batch, n_vocab, device):
    need = int(load_library().mli_decoder_sampled_scratch_bytes(n_batch, n_vocab))
    return torch.empty(max(need, 16), dtype=torch.uint8, device=device), need


def decoder_sampled(batch_result, emb_table, wpe_table, inp_embedding, lengths, decoder_result, temperature, top_k,
                    top_p, seed):
    """EXTENSION: decoder_fused with the sampled head (mli_decoder_sampled): logits GEMM, draw, length update, next
    embedding."""
    B, D = batch_result.shape
    sc, need = _sampled_scratch(B, emb_table.shape[0], batch_result.device)
    _check(load_library().mli_decoder_sampled(_p(batch_result), _p(emb_table), _p(wpe_table), _p(inp_embedding),
                                              _p(lengths), _p(decoder_result), B, emb_table.shape[0],
                                              wpe_table.shape[0], D, *_sampling_args(temperature, top_k, top_p, seed),
                                              _p(sc), need, _stream()), "mli_decoder_sampled")


def paged_decoder_sampled(batch_result, emb_table, wpe_table, page_table, lengths, decoder_result, i_decoder, elem,
                          temperature, top_k, top_p, seed):
    """EXTENSION: paged_decoder_fused with the sampled head (mli_paged_decoder_sampled)."""
    B, D = batch_result.shape
    n_res = decoder_result.shape[1] if decoder_result.dim() == 2 else 1
    sc, need = _sampled_scratch(B, emb_table.shape[0], batch_result.device)
    _check(load_library().mli_paged_decoder_sampled(_p(batch_result), _p(emb_table), _p(wpe_table), _p(page_table),
                                                    _p(lengths), _p(decoder_result), B, emb_table.shape[0],
                                                    wpe_table.shape[0], D, n_res, i_decoder, int(elem),
                                                    *_sampling_args(temperature, top_k, top_p, seed), _p(sc), need,
                                                    _stream()), "mli_paged_decoder_sampled")


def _logprob_outputs(decoder_result, n_top):
    """token_logprob, top_ids, top_logprobs shaped and strided like decoder_result ([B] or [B, n_results])"""
    shape, dev = tuple(decoder_result.shape), decoder_result.device
    return (torch.empty(shape, dtype=torch.float32, device=dev), torch.empty(shape + (n_top,), dtype=torch.int32, device=dev),
            torch.empty(shape + (n_top,), dtype=torch.float32, device=dev))


def decoder_sampled_logprobs(batch_result, emb_table, wpe_table, inp_embedding, lengths, decoder_result, i_decoder,
                             temperature, top_k, top_p, seed, n_top=0):
    """EXTENSION: decoder_sampled plus the log-probabilities of sample_tokens_logprobs (mli_decoder_sampled_logprobs);
    decoder_result [B] or [B, n_results], written at column i_decoder.  Returns (token_logprob, top_ids, top_logprobs),
    shaped like decoder_result (+ [n_top])."""
    B, D = batch_result.shape
    n_res = decoder_result.shape[1] if decoder_result.dim() == 2 else 1
    lp, ids, tops = _logprob_outputs(decoder_result, int(n_top))
    sc, need = _sampled_scratch(B, emb_table.shape[0], batch_result.device)
    _check(load_library().mli_decoder_sampled_logprobs(
        _p(batch_result), _p(emb_table), _p(wpe_table), _p(inp_embedding), _p(lengths), _p(decoder_result), B,
        emb_table.shape[0], wpe_table.shape[0], D, n_res, i_decoder, *_sampling_args(temperature, top_k, top_p, seed),
        _p(lp), _p(ids) if n_top else None, _p(tops) if n_top else None, int(n_top), _p(sc), need, _stream()),
        "mli_decoder_sampled_logprobs")
    return lp, ids, tops


def paged_decoder_sampled_logprobs(batch_result, emb_table, wpe_table, page_table, lengths, decoder_result, i_decoder, elem,
                                   temperature, top_k, top_p, seed, n_top=0):
    """EXTENSION: paged_decoder_sampled plus the log-probabilities (mli_paged_decoder_sampled_logprobs)."""
    B, D = batch_result.shape
    n_res = decoder_result.shape[1] if decoder_result.dim() == 2 else 1
    lp, ids, tops = _logprob_outputs(decoder_result, int(n_top))
    sc, need = _sampled_scratch(B, emb_table.shape[0], batch_result.device)
    _check(load_library().mli_paged_decoder_sampled_logprobs(
        _p(batch_result), _p(emb_table), _p(wpe_table), _p(page_table), _p(lengths), _p(decoder_result), B,
        emb_table.shape[0], wpe_table.shape[0], D, n_res, i_decoder, int(elem),
        *_sampling_args(temperature, top_k, top_p, seed), _p(lp), _p(ids) if n_top else None,
        _p(tops) if n_top else None, int(n_top), _p(sc), need, _stream()), "mli_paged_decoder_sampled_logprobs")
    return lp, ids, tops


def stream_wait_stream(waiter, signaller):
    """torch streams: `waiter` waits for everything queued on `signaller` so far (mli_stream_wait_stream)."""
    _check(load_library().mli_stream_wait_stream(ctypes.c_void_p(waiter.cuda_stream), ctypes.c_void_p(signaller.cuda_stream)),
           "mli_stream_wait_stream")


class StepGraph:
    """hipGraph of whatever `fn` launches on the current (non-default) stream: mli_graph_* of the C ABI.  Everything
    `fn` touches must already be allocated (workspaces included): call it once eagerly first."""

    def __init__(self, fn):
        lib = load_library()
        stream = _stream()
        _check(lib.mli_graph_begin_capture(stream), "mli_graph_begin_capture")
        try:
            fn()
        finally:
            handle = ctypes.c_void_p()
            rc = lib.mli_graph_end_capture(stream, ctypes.byref(handle))
        _check(rc, "mli_graph_end_capture")
        self._exec = handle

    def launch(self):
        _check(load_library().mli_graph_launch(self._exec, _stream()), "mli_graph_launch")

    def close(self):
        if self._exec:
            load_library().mli_graph_destroy(self._exec)
            self._exec = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- encoder / decoder ---------------------------------------------------------------------
def launch_inference_optimized_encoder_kernel(emb_table, wpe, inp, inp_embedding, lengths, new_item_indices,
                                              n_new_items):
    B, S, D = inp_embedding.shape
    _check(load_library().mli_inference_optimized_encoder(_p(emb_table), _p(wpe), _p(inp), _p(inp_embedding),
                                                          _p(lengths), _p(new_item_indices), B, S, D, n_new_items,
                                                          _stream()), "mli_inference_optimized_encoder")


def launch_paged_attention_encoder_kernel(emb_table, wpe, inp, page_table, lengths, new_item_indices, n_new_items):
    B, S = inp.shape
    _check(load_library().mli_paged_attention_encoder(_p(emb_table), _p(wpe), _p(inp), _p(page_table), _p(lengths),
                                                      _p(new_item_indices), B, S, emb_table.shape[1], n_new_items,
                                                      _stream()), "mli_paged_attention_encoder")


def launch_decoder(batch_result, emb_table, emb_score, wpe_table, inp_embedding, lengths, decoder_result):
    B, D = batch_result.shape
    _check(load_library().mli_decoder(_p(batch_result), _p(emb_table), _p(emb_score), _p(wpe_table),
                                      _p(inp_embedding), _p(lengths), _p(decoder_result), B, emb_table.shape[0],
                                      wpe_table.shape[0], D, _stream()), "mli_decoder")


def launch_paged_attention_decoder_multi_rounds(batch_result, emb_table, emb_score, wpe_table, page_table, lengths,
                                                decoder_result, i_decoder):
    B, D = batch_result.shape
    n_res = decoder_result.shape[1] if decoder_result.dim() == 2 else 1
    _check(load_library().mli_paged_decoder_multi_rounds(_p(batch_result), _p(emb_table), _p(emb_score),
                                                         _p(wpe_table), _p(page_table), _p(lengths),
                                                         _p(decoder_result), B, emb_table.shape[0],
                                                         wpe_table.shape[0], D, n_res, i_decoder, _stream()),
           "mli_paged_decoder_multi_rounds")


def launch_paged_attention_cublas_decoder_multi_rounds(batch_result, emb_table, emb_score, wpe_table, page_table, lengths,
                                                       decoder_result, i_decoder, handle=None):
    """decoder.h:32-37: the same head with a cublasHandle_t at the end (a GemmHandle here; nothing to hand to MFMA)."""
    assert handle is None or isinstance(handle, GemmHandle)
    launch_paged_attention_decoder_multi_rounds(batch_result, emb_table, emb_score, wpe_table, page_table, lengths,
                                                decoder_result, i_decoder)


# ---- test / measurement support -------------------------------------------------------------
def launch_clone_inp_embedding_k_v_cache(page_table, inp_embedding, kt_cache, v_cache, lengths):
    B, S, D = inp_embedding.shape
    _check(load_library().mli_clone_inp_embedding_k_v_cache(_p(page_table), _p(inp_embedding), _p(kt_cache),
                                                            _p(v_cache), _p(lengths), B, S, D, _stream()),
           "mli_clone_inp_embedding_k_v_cache")


def stream_copy(src, dst):
    _check(load_library().mli_stream_copy(_p(src), _p(dst), src.numel(), _stream()), "mli_stream_copy")


def stream_read(src, sink):
    _check(load_library().mli_stream_read(_p(src), _p(sink), src.numel(), _stream()), "mli_stream_read")


def f32_to_fp8(src, dst=None):
    """float32 tensor -> uint8 tensor of OCP e4m3 codes with the kernels' own conversion (mli_f32_to_fp8)."""
    if dst is None:
        dst = torch.empty(src.shape, dtype=torch.uint8, device=src.device)
    _check(load_library().mli_f32_to_fp8(_p(src), _p(dst), src.numel(), _stream()), "mli_f32_to_fp8")
    return dst


def get_latest_k_q_v_paged_lean(page_table, lengths, wk, wq, wv, q_output, n_sequence, elem=None, n_heads=1, rope=None):
    """The decode projection for any page element type (mli_get_latest_k_q_v_paged_lean).  rope given (a [n_sequence,
    D / n_heads / 2, 2] float32 (cos, sin) table on the device): k and q are rotated by slot L - 1
    (mli_get_latest_k_q_v_paged_rope)."""
    B = page_table.shape[0]
    if rope is not None:
        _check(load_library().mli_get_latest_k_q_v_paged_rope(_p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv), _p(q_output),
                                                              B, n_sequence, wq.shape[0], int(n_heads), _p(rope),
                                                              _elem_of(wk, elem), _stream()),
               "mli_get_latest_k_q_v_paged_rope")
        return
    _check(load_library().mli_get_latest_k_q_v_paged_lean(_p(page_table), _p(lengths), _p(wk), _p(wq), _p(wv), _p(q_output), B,
                                                          n_sequence, wq.shape[0], _elem_of(wk, elem), _stream()),
           "mli_get_latest_k_q_v_paged_lean")


def fill_new_k_v_cache_paged_rope(page_table, new_batch_idx, lengths, wk, wv, n_new_items, n_sequence, n_heads, rope, elem=None):
    """The prefill fill reading x from the pages, K rotated by the token's slot (mli_fill_new_k_v_cache_paged_rope)."""
    B = page_table.shape[0]
    _check(load_library().mli_fill_new_k_v_cache_paged_rope(_p(page_table), _p(new_batch_idx), _p(lengths), _p(wk), _p(wv), B,
                                                            n_sequence, wk.shape[0], n_new_items, int(n_heads), _p(rope),
                                                            _elem_of(wk, elem), _stream()),
           "mli_fill_new_k_v_cache_paged_rope")
