"""ctypes front end of the engine C ABI (include/mli_engine.h): continuous batching on one GPU.

Mirrors how the reference's drivers use the engine (tests/paged_for_profile.cpp:10-62): build the item queue
and the model, then run start_*_engine to completion.  Nothing is computed in Python.
"""
import ctypes
import math

import numpy as np

from ._lib import EngineConfig, EnginePageStats, EngineStats, MliError, ShardStats, load_library

CONTIGUOUS, PAGED, PAGED_GEMM, PAGED_BF16 = 0, 1, 2, 3  # PAGED_BF16: extension, bf16 pages and weights
PAGED_FP8 = 4  # extension, opt-in: fp8 (OCP e4m3) pages, bf16 weights


def _fp(a):
    a = np.ascontiguousarray(a, dtype=np.float32)
    return a, a.ctypes.data_as(ctypes.c_void_p)


def sampling_params(temperature=0.0, top_k=0, top_p=1.0, seed=0):
    """Checked (temperature, top_k, top_p, seed) for mli_engine_add_item_sampled, or None when every argument is at its
    default (greedy: the plain entry point).  Raises ValueError where the library would refuse the item."""
    if (temperature, top_k, top_p, seed) == (0.0, 0, 1.0, 0):
        return None
    temperature, top_p = float(temperature), float(top_p)
    if not math.isfinite(temperature) or temperature < 0:
        raise ValueError(f"temperature must be finite and >= 0, got {temperature}")
    if int(top_k) != top_k or top_k < 0:
        raise ValueError(f"top_k must be an integer >= 0, got {top_k}")
    if not 0.0 < top_p <= 1.0:
        raise ValueError(f"top_p must lie in (0, 1], got {top_p}")
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ValueError(f"seed must be an integer in [0, 2**64), got {seed}")
    return temperature, int(top_k), top_p, int(seed)


class Engine:
    def __init__(self, kind, n_batch, n_sequence, emb_dim, n_vocab, emb_table, pos_table, wk, wq, wv, n_blocks=0,
                 n_forward_rounds=1, device=0, reference_length_reset_quirk=False, n_heads=1, window=None, sinks=None,
                 release_pages=False, n_kv_heads=None, logprobs=None, prompt_logprobs=False, alibi=None,
                 rope=None, softcap=None, sink_logits=None):
        self._lib = load_library()
        self.cfg = EngineConfig(kind, n_batch, n_sequence, emb_dim, n_vocab, n_blocks, n_forward_rounds, device,
                                int(reference_length_reset_quirk))
        keep = [_fp(x) for x in (emb_table, pos_table, wk, wq, wv)]
        assert keep[0][0].shape == (n_vocab, emb_dim) and keep[1][0].shape == (n_sequence, emb_dim)
        self._h = ctypes.c_void_p()
        self._check(self._lib.mli_engine_create(ctypes.byref(self.cfg), *[k[1] for k in keep], ctypes.byref(self._h)))
        if n_heads != 1:
            self.set_heads(n_heads)
        if n_kv_heads is not None:
            self.set_kv_heads(n_kv_heads)
        if window is not None:
            self.set_window(window)
        if sinks is not None:
            self.set_sinks(sinks)
        if release_pages:
            self.set_page_release(True)
        if logprobs is not None:
            self.set_logprobs(logprobs)
        if prompt_logprobs:
            self.set_prompt_logprobs(True)
        if alibi is not None and alibi is not False:
            self.set_alibi(None if alibi is True else alibi)
        if rope is not None and rope is not False:
            self.set_rope(10000.0 if rope is True else rope)
        if softcap is not None:
            self.set_softcap(softcap)
        if sink_logits is not None:
            self.set_sink_logits(sink_logits)

    def _check(self, rc):
        if rc != 0:
            raise MliError("Hip Failure: " + (self._lib.mli_engine_last_error() or b"").decode())

    def set_heads(self, n_heads):
        """Multi-head attention (mli_engine_set_heads): before the first step or run, fp32 / bf16 paged kinds."""
        self._check(self._lib.mli_engine_set_heads(self._h, int(n_heads)))

    def set_kv_heads(self, n_kv_heads):
        """Grouped-query attention (mli_engine_set_kv_heads): `n_kv_heads` K/V heads, a divisor of the engine's n_heads,
        serve the query heads; only the first n_kv_heads * emb_dim / n_heads output columns of wk / wv matter.  Before the
        first step or run, fp32 / bf16 paged kinds; n_kv_heads == n_heads changes nothing."""
        self._check(self._lib.mli_engine_set_kv_heads(self._h, int(n_kv_heads)))

    def set_alibi(self, slopes=None):
        """ALiBi (mli_engine_set_alibi): every decode scan adds slopes[h] * (s - (L - 1)) to query head h's scaled scores.
        slopes: one finite value per head of the engine's n_heads (>= 2), or None for the standard slopes
        (ops.alibi_slopes).  Before the first step or run, fp32 / bf16 paged kinds, not with prompt log-probabilities."""
        if slopes is None:
            self._check(self._lib.mli_engine_set_alibi(self._h, None, 0))
            return
        a = np.ascontiguousarray(slopes, dtype=np.float32).reshape(-1)
        self._check(self._lib.mli_engine_set_alibi(self._h, a.ctypes.data_as(ctypes.c_void_p), int(a.size)))

    def set_softcap(self, cap):
        """Attention logit soft-capping (mli_engine_set_softcap): every decode scan -- and the prompt scan of an engine with
        prompt log-probabilities -- replaces a scaled score x by cap * tanh(x / cap).  cap: finite and > 0; 0 turns it off.
        Before the first step or run, fp32 / bf16 paged kinds with n_heads >= 2 and lean layers, not with ALiBi."""
        self._check(self._lib.mli_engine_set_softcap(self._h, float(cap)))

    def set_sink_logits(self, values):
        """Learned attention-sink logits (mli_engine_set_sink_logits): values[h] takes part in query head h's softmax as one
        more logit without a value row, in every decode scan and in the prompt scan of an engine with prompt log-probabilities.
        values: n_heads floats, each finite or -inf (-inf: no sink for that head); None turns the switch off.  Before the
        first step or run, fp32 / bf16 paged kinds with n_heads >= 2 and lean layers, not with ALiBi or a soft cap."""
        if values is None:
            self._check(self._lib.mli_engine_set_sink_logits(self._h, None, 0))
            return
        a = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        self._check(self._lib.mli_engine_set_sink_logits(self._h, a.ctypes.data_as(ctypes.c_void_p), int(a.size)))

    def set_rope(self, rope=10000.0):
        """Rotary position embeddings (mli_engine_set_rope / mli_engine_set_rope_table): prefill and projection rotate K and q
        by the token's absolute slot.  rope: theta (a number: the standard table for the engine's current n_heads), or a table
        of n_sequence * head_dim floats ([n_sequence, head_dim // 2, 2] (cos, sin), e.g. ops.rope_table or a scaled variant).
        Before the first step or run, paged kinds with lean layers, not with prompt log-probabilities; pass a zero
        pos_table."""
        if np.isscalar(rope):
            self._check(self._lib.mli_engine_set_rope(self._h, float(rope)))
            return
        a = np.ascontiguousarray(rope, dtype=np.float32).reshape(-1)
        self._check(self._lib.mli_engine_set_rope_table(self._h, a.ctypes.data_as(ctypes.c_void_p), int(a.size)))

    def set_window(self, window):
        """Sliding-window attention (mli_engine_set_window): every row attends its newest `window` tokens.  Before the
        first step or run, paged kinds; window >= n_sequence changes nothing."""
        self._check(self._lib.mli_engine_set_window(self._h, int(window)))

    def set_sinks(self, n_sink):
        """Attention sinks (mli_engine_set_sinks): beside the window every row keeps its first `n_sink` tokens attended.
        Before the first step or run, paged kinds; without a window below n_sequence it changes nothing."""
        self._check(self._lib.mli_engine_set_sinks(self._h, int(n_sink)))

    def set_page_release(self, enabled=True):
        """Early page release (mli_engine_set_page_release): beside a window, rows return the pages below it to the pool
        while they decode, and new rows take and prefill their live pages only.  Before the first step or run, paged
        kinds; without a window below n_sequence it changes nothing."""
        self._check(self._lib.mli_engine_set_page_release(self._h, int(bool(enabled))))

    def set_logprobs(self, n_top=0):
        """Per-token log-probabilities (mli_engine_set_logprobs): the engine records, for every generated
        token, its natural-log probability under the raw model distribution and the `n_top` (0 .. 8) most probable
        alternatives.  Before the first step or run, every kind; item ids must be unique from then on."""
        self._check(self._lib.mli_engine_set_logprobs(self._h, int(n_top)))
        self._n_top = int(n_top)

    def finished_logprobs(self):
        """{id: (n_prompt, logprobs [n], top_ids [n, n_top], top_logprobs [n, n_top])} of the finished items: entry i
        belongs to token n_prompt + i of finished()'s tokens (mli_engine_get_finished_logprobs)."""
        out = {}
        n_top = getattr(self, "_n_top", 0)
        cap = self.cfg.n_sequence + 16
        lp = np.empty(cap, np.float32)
        ids = np.empty(cap * max(n_top, 1), np.int32)
        tops = np.empty(cap * max(n_top, 1), np.float32)
        for i, (item_id, _) in enumerate(self.finished()):
            n_prompt, n = ctypes.c_int(), ctypes.c_int()
            self._check(self._lib.mli_engine_get_finished_logprobs(
                self._h, i, ctypes.byref(n_prompt), lp.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n),
                ids.ctypes.data_as(ctypes.c_void_p), tops.ctypes.data_as(ctypes.c_void_p), cap * n_top))
            k = n.value
            out[item_id] = (n_prompt.value, lp[:k].copy(), ids[:k * n_top].reshape(k, n_top).copy(),
                            tops[:k * n_top].reshape(k, n_top).copy())
        return out

    def set_prompt_logprobs(self, enabled=True):
        """Prompt log-probabilities (mli_engine_set_prompt_logprobs): the engine also reports, for every prompt
        token but the first, its log-probability after the tokens before it and the alternatives there.  After
        set_logprobs (which supplies n_top), before the first step or run; fp32 / bf16 paged kinds, not with page release."""
        self._check(self._lib.mli_engine_set_prompt_logprobs(self._h, int(bool(enabled))))

    def finished_prompt_logprobs(self):
        """{id: (logprobs [n], top_ids [n, n_top], top_logprobs [n, n_top])} of the finished items: entry i belongs to prompt
        token i + 1, n = n_prompt - 1 (mli_engine_get_finished_prompt_logprobs)."""
        out = {}
        n_top = getattr(self, "_n_top", 0)
        cap = self.cfg.n_sequence + 16
        lp = np.empty(cap, np.float32)
        ids = np.empty(cap * max(n_top, 1), np.int32)
        tops = np.empty(cap * max(n_top, 1), np.float32)
        for i, (item_id, _) in enumerate(self.finished()):
            n = ctypes.c_int()
            self._check(self._lib.mli_engine_get_finished_prompt_logprobs(
                self._h, i, lp.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n), ids.ctypes.data_as(ctypes.c_void_p),
                tops.ctypes.data_as(ctypes.c_void_p), cap * n_top))
            k = n.value
            out[item_id] = (lp[:k].copy(), ids[:k * n_top].reshape(k, n_top).copy(), tops[:k * n_top].reshape(k, n_top).copy())
        return out

    def page_stats(self):
        """mli_engine_get_page_stats: pool_pages, in_use, peak_in_use, released_early, preemptions (paged kinds)."""
        st = EnginePageStats()
        self._check(self._lib.mli_engine_get_page_stats(self._h, ctypes.byref(st)))
        return st

    def use_private_stream(self):
        self._check(self._lib.mli_engine_use_private_stream(self._h))

    def configure(self, lean_layers=None, step_graphs=None):
        """This engine's own composition / replay switches (mli_engine_configure); None leaves a value as it is."""
        self._check(self._lib.mli_engine_configure(self._h, -1 if lean_layers is None else int(lean_layers),
                                                   -1 if step_graphs is None else int(step_graphs)))

    def set_pipelined(self, enabled=True):
        self._check(self._lib.mli_engine_set_pipelined(self._h, int(enabled)))

    def add_item(self, item_id, tokens, temperature=0.0, top_k=0, top_p=1.0, seed=0):
        """Queue an item.  With every sampling argument at its default it is decoded greedily by the plain entry point;
        otherwise by mli_engine_add_item_sampled (temperature 0 is still greedy)."""
        params = sampling_params(temperature, top_k, top_p, seed)
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        if params is None:
            self._check(self._lib.mli_engine_add_item(self._h, int(item_id), t.ctypes.data_as(ctypes.c_void_p), len(t)))
        else:
            self._check(self._lib.mli_engine_add_item_sampled(self._h, int(item_id), t.ctypes.data_as(ctypes.c_void_p),
                                                              len(t), *params))

    def run(self):
        st = EngineStats()
        self._check(self._lib.mli_engine_run(self._h, ctypes.byref(st)))
        return st

    def step(self):
        done = ctypes.c_int(0)
        self._check(self._lib.mli_engine_step(self._h, ctypes.byref(done)))
        return bool(done.value)

    def stats(self):
        st = EngineStats()
        self._check(self._lib.mli_engine_get_stats(self._h, ctypes.byref(st)))
        return st

    def decoder_result_ptr(self):
        p = ctypes.c_void_p()
        n = ctypes.c_int()
        self._check(self._lib.mli_engine_decoder_result(self._h, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def finished(self):
        """[(id, tokens)] in completion order."""
        out = []
        cap = self.cfg.n_sequence + 16
        buf = np.empty(cap, np.int32)
        for i in range(self.stats().finished):
            item_id = ctypes.c_int()
            n = ctypes.c_int()
            self._check(self._lib.mli_engine_get_finished(self._h, i, ctypes.byref(item_id),
                                                          buf.ctypes.data_as(ctypes.c_void_p), cap, ctypes.byref(n)))
            out.append((item_id.value, buf[:n.value].copy()))
        return out

    def close(self):
        if self._h:
            self._lib.mli_engine_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedEngine(Engine):
    """An engine owned by a ShardGroup: same accessors, never destroyed from here."""

    def __init__(self, lib, handle, cfg):
        self._lib, self._h, self.cfg = lib, ctypes.c_void_p(handle), cfg

    def close(self):
        self._h = ctypes.c_void_p()


class ShardGroup:
    """include/mli_shard.h: one engine per GPU inside this process (one host thread each), stepped in lock step with one RCCL
    all-gather of the generated token ids per rank and iteration.  `n_batch` / `n_blocks` are PER RANK."""

    def __init__(self, kind, n_batch, n_sequence, emb_dim, n_vocab, emb_table, pos_table, wk, wq, wv, devices, n_blocks=0,
                 n_forward_rounds=1, loopback_ranks=0):
        """devices: one ordinal per rank (RCCL communicator); or loopback_ranks = N: N ranks on devices[0], exchange by
        device-to-device copies (mli_shard_group_create_loopback)."""
        self._lib = load_library()
        self.devices = [int(d) for d in devices]
        self.cfg = EngineConfig(kind, n_batch, n_sequence, emb_dim, n_vocab, n_blocks, n_forward_rounds, 0, 0)
        keep = [_fp(x) for x in (emb_table, pos_table, wk, wq, wv)]
        dev = np.asarray(self.devices, dtype=np.int32)
        self._h = ctypes.c_void_p()
        if loopback_ranks:
            self._check(self._lib.mli_shard_group_create_loopback(ctypes.byref(self.cfg), int(loopback_ranks), self.devices[0],
                                                                  *[k[1] for k in keep], ctypes.byref(self._h)))
            self.devices = [self.devices[0]] * int(loopback_ranks)
            return
        self._check(self._lib.mli_shard_group_create(ctypes.byref(self.cfg), len(self.devices),
                                                     dev.ctypes.data_as(ctypes.c_void_p), *[k[1] for k in keep],
                                                     ctypes.byref(self._h)))

    def _check(self, rc):
        if rc != 0:
            raise MliError("Hip Failure: " + (self._lib.mli_shard_last_error() or b"").decode())

    def add_item(self, item_id, tokens):
        t = np.ascontiguousarray(tokens, dtype=np.int32)
        self._check(self._lib.mli_shard_group_add_item(self._h, int(item_id), t.ctypes.data_as(ctypes.c_void_p), len(t)))

    def run(self):
        st = ShardStats()
        self._check(self._lib.mli_shard_group_run(self._h, ctypes.byref(st)))
        return st

    def gathered_ptr(self, rank):
        p, n = ctypes.c_void_p(), ctypes.c_int()
        self._check(self._lib.mli_shard_group_gathered(self._h, rank, ctypes.byref(p), ctypes.byref(n)))
        return p.value, n.value

    def engine(self, rank):
        h = self._lib.mli_shard_group_engine(self._h, rank)
        if not h:
            raise MliError("no such rank")
        return _BorrowedEngine(self._lib, h, self.cfg)

    def close(self):
        if self._h:
            self._lib.mli_shard_group_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
