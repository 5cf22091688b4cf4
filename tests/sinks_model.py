"""Attention sinks beside the sliding window, for the tests: with window W and n_sink K a row of length L
attends the slots s < L with s < K or s >= lo, lo = max(0, L - W) -- its first K tokens and its newest W; a row with
lo <= K attends all of [0, L).  That is the un-windowed problem on the attended slots, so the references are built as
window_model builds its own: per row the attended slots of K and V are moved to the front (window_model.compact with the
sink-plus-window mask), and heads_model.oracle_heads (the fp32 CPU oracle per head) and heads_model.HeadsModel (float64 per
head) are applied unchanged.  Errors, tolerance and the per-family comparison are heads_model.compare's.

Score families are applied to the FULL row before slicing, so `early_peak` puts its +30 tokens on slots 0 .. 15: on the
sinks (gross when they are dropped) and on the gap slots that share the sinks' last page (gross when they are attended).

TEST INFRASTRUCTURE, like window_model.py and heads_model.py: never used by the product."""
import numpy as np

import heads_model as hm
import window_model as wm
from engine_sim import CpuEngine
from helpers import PAGE

# (seed, B, S, D, heads, page types, (W, K) pairs, forced chunk_tokens): the smallest shapes at which each mechanism of the
# scan with sinks can still go wrong (tests/test_sinks_scan_gpu.py says which).  fp8 pages exist with one head only.
SINK_SHAPES = [
    (501, 40, 64, 64, (1, 2), ("f32", "bf16", "fp8"), ((5, 1), (16, 4), (17, 16), (8, 17), (33, 20)), (0,)),
    (502, 24, 256, 512, (1, 8), ("f32", "bf16", "fp8"), ((40, 4), (100, 20)), (0, 256)),
    (503, 20, 1024, 256, (1, 2), ("f32", "bf16"), ((513, 4),), (0,)),
    (504, 24, 512, 1024, (1, 8), ("bf16", "fp8"), ((130, 4),), (0,)),
    (505, 8, 256, 2048, (1,), ("f32", "bf16", "fp8"), ((100, 4),), (0,)),
    (506, 700, 128, 64, (1, 2), ("f32",), ((50, 4),), (0,)),
]


def sink_pages(K):
    return -(-int(K) // PAGE)


def skipped_pages(lengths, W, K):
    """pages dropped between the sink pages and the window's first page, per row"""
    return np.maximum(wm.window_lo(lengths, W) // PAGE - sink_pages(K), 0)


def sink_mask(lengths, S, W, K):
    s = np.arange(S)[None, :]
    L = np.asarray(lengths).astype(np.int64)[:, None]
    lo = np.maximum(L - int(W), 0)
    return (s < L) & ((s < int(K)) | (s >= lo))


def wanted_lengths(S, W, K):
    """The lengths every case must contain, as far as they fit a row: 0, 1, K - 1, K, K + 1, S - 1; K + W - 1 .. K + W + 1
    (the first row with a gap is K + W + 1); W + 15 .. W + 17; and the lengths that put lo at the end of the last sink page
    (the hole inside a page), at the start of the page after it and one slot in (the hole up to and across a page edge,
    nothing skipped), and at the start of the page after that and one slot in (one page skipped)."""
    ps = sink_pages(K)
    los = [PAGE * ps - 1, PAGE * ps, PAGE * ps + 1, PAGE * (ps + 1), PAGE * (ps + 1) + 1]
    want = [0, 1, K - 1, K, K + 1, S - 1, K + W - 1, K + W, K + W + 1, W + 15, W + 16, W + 17] + [lo + W for lo in los]
    return sorted({e for e in want if 0 <= e <= S - 1})


def sink_lengths(seed, B, S, W, K):
    """A list of length vectors for the case.  Normally one: the wanted lengths in the first rows, random rows behind
    them, half of them long enough to have a gap.  A batch with fewer rows than wanted lengths (B = 8) gets several
    vectors, each with 0 and S - 1 and its share of the rest, dealt round-robin so that every vector has rows with a gap."""
    want = wanted_lengths(S, W, K)
    rng = np.random.default_rng(seed + 9300)
    if B >= len(want) + 6:
        L = rng.integers(0, S, size=B).astype(np.int32)
        L[:len(want)] = want
        free = np.arange(len(want), B)
        gap_from = min(K + W + PAGE + 1, S - 1)
        L[free[::2]] = rng.integers(gap_from, S, size=len(free[::2]))
        parts = [L]
    else:
        rest = [e for e in want if e not in (0, S - 1)]
        n = -(-len(rest) // (B - 2))
        parts = []
        for i in range(n):
            share = rest[i::n]
            share += rng.integers(K + W + 1, S, size=B - 2 - len(share)).tolist()
            parts.append(np.asarray([0] + share + [S - 1], np.int32))
    have = set(np.concatenate(parts).tolist())
    assert have >= set(want), sorted(set(want) - have)
    for L in parts:
        assert L.min() == 0 and L.max() == S - 1 and len(L) == B
        assert (wm.window_lo(L, W) > K).any(), "every vector has a row with a gap"
    allL = np.concatenate(parts)
    if S - 1 >= W + PAGE * (sink_pages(K) + 1) + 1:
        skip, lo = skipped_pages(allL, W, K), wm.window_lo(allL, W)
        assert ((skip == 0) & (lo // PAGE == sink_pages(K) - 1)).any() and ((skip == 0) & (lo // PAGE == sink_pages(K))).any()
        assert (skip == 1).any()
    return parts


def gap_offsets(table, lengths, S, D, W, K):
    """Pool offsets (in elements) of the K and V segments of the gap slots K <= s < lo of every row."""
    lo = wm.window_lo(lengths, W)
    s = np.arange(S)[None, :]
    b_idx, s_idx = np.nonzero((s >= int(K)) & (s < lo[:, None]))
    page = table[b_idx, s_idx // PAGE]
    assert (page >= 0).all()
    off = page.astype(np.int64) + (s_idx % PAGE) * 3 * D + D
    return (off[:, None] + np.arange(2 * D)[None, :]).reshape(-1)


def gap_pages(lengths, n_pages, W, K):
    """[B, n_pages] bool: the pages wholly inside the gap, whose page-table entries are never read"""
    p0 = wm.window_lo(lengths, W) // PAGE
    p = np.arange(n_pages)[None, :]
    return (p >= sink_pages(K)) & (p < p0[:, None])


def sink_slice(kt, v, lengths, W, K):
    return wm.compact(kt, v, lengths, sink_mask(lengths, kt.shape[2], W, K))


def oracle_sinks(oracle, q, kt, v, lengths, H, W, K):
    kt2, v2, L2 = sink_slice(kt, v, lengths, W, K)
    return hm.oracle_heads(oracle, q, kt2, v2, L2, H)


def model_sinks(q, kt, v, lengths, H, W, K):
    kt2, v2, L2 = sink_slice(kt, v, lengths, W, K)
    return hm.HeadsModel(q, kt2, v2, L2, H)


# ---- wrong models: the faults a scan with sinks actually has, each as the set of slots it attends --------------------------
def _parts(lengths, S, W):
    s = np.arange(S)[None, :]
    L = np.asarray(lengths).astype(np.int64)[:, None]
    return s, L, np.maximum(L - int(W), 0)


def mask_sinks_ignored(lengths, S, W, K):
    return wm.window_mask(lengths, S, W)


def mask_one_sink_too_many(lengths, S, W, K):
    return sink_mask(lengths, S, W, K + 1)


def mask_one_sink_too_few(lengths, S, W, K):
    return sink_mask(lengths, S, W, K - 1)


def mask_sinks_page_granular(lengths, S, W, K):
    """K rounded up to a page"""
    return sink_mask(lengths, S, W, PAGE * sink_pages(K))


def mask_window_shrunk_by_sinks(lengths, S, W, K):
    """the newest W - K tokens beside the sinks: K + (W - K) = W tokens in all"""
    return sink_mask(lengths, S, max(W - K, 0), K)


def mask_gap_in_shared_pages_attended(lengths, S, W, K):
    """the hole masked by pages only: the rest of the last sink page and the window's first page below lo are attended"""
    s, L, lo = _parts(lengths, S, W)
    return (s < L) & ((s < PAGE * sink_pages(K)) | (s >= lo // PAGE * PAGE))


def mask_sink_mask_on_every_page(lengths, S, W, K):
    """the sink mask of a page taken as t < K % 16 on every page of the virtual row instead of t < K - 16 P"""
    s, L, lo = _parts(lengths, S, W)
    in_row = (s < PAGE * sink_pages(K)) | (s >= lo // PAGE * PAGE)
    return (s < L) & in_row & ((s % PAGE < K % PAGE) | (s >= lo))


def mask_sinks_at_the_windows_origin(lengths, S, W, K):
    """the sink pages read where the window's pages start: slots [16 p0, 16 p0 + K) instead of [0, K)"""
    s, L, lo = _parts(lengths, S, W)
    origin = lo // PAGE * PAGE
    shifted = (s < L) & (((s >= origin) & (s < origin + K)) | (s >= lo))
    return np.where(lo <= K, s < L, shifted)


WRONG_MASKS = {"sinks ignored": mask_sinks_ignored, "K + 1": mask_one_sink_too_many, "K - 1": mask_one_sink_too_few,
               "K rounded up to a page": mask_sinks_page_granular, "window shrunk to W - K": mask_window_shrunk_by_sinks,
               "gap inside a shared page attended": mask_gap_in_shared_pages_attended,
               "sink mask t < K % 16 on every page": mask_sink_mask_on_every_page,
               "sink pages read at the window's origin": mask_sinks_at_the_windows_origin}


def wrong_model(name, q, kt, v, lengths, H, W, K):
    """(float64 attention [B, D] of the wrong model, whether it attends other slots than the right one on any row)"""
    S = kt.shape[2]
    L = np.asarray(lengths).astype(np.int64)[:, None]
    mask = WRONG_MASKS[name](lengths, S, W, K) & (np.arange(S)[None, :] < L)
    differs = bool((mask != sink_mask(lengths, S, W, K)).any())
    kt2, v2, L2 = wm.compact(kt, v, lengths, mask)
    return hm.HeadsModel(q, kt2, v2, L2, H).o, differs


# ---- the CPU engine with heads, a window and sinks ---------------------------------------------------------------------------
class _SinksOracle(hm._HeadsOracle):
    """heads_model._HeadsOracle whose attention sees the first `n_sink` and the newest `window` tokens of every row only."""

    def __init__(self, oracle, n_heads, window, n_sink):
        super().__init__(oracle, n_heads)
        self._W, self._K = window, n_sink

    def _attend(self, q, kt, v, lengths, att):
        att[...] = oracle_sinks(self._o, q, kt, v, lengths, self._H, self._W, self._K)


class SinksCpuEngine(CpuEngine):
    def __init__(self, oracle, model, items, n_batch, n_sequence, n_heads, window, n_sink, bf16=False):
        self.sinks_oracle = _SinksOracle(oracle, n_heads, window, n_sink)
        super().__init__(self.sinks_oracle, model, items, n_batch, n_sequence, bf16=bf16)


def run_sinks_cpu_engine(oracle, model, items, n_batch, n_sequence, n_heads, window, n_sink, bf16=False):
    """({item id: all tokens}, smallest top-2 logit gap of the run)."""
    e = SinksCpuEngine(oracle, model, items, n_batch, n_sequence, n_heads, window, n_sink, bf16=bf16)
    while not e.done():
        e.step()
    return e.finished, e.sinks_oracle.min_logit_gap
