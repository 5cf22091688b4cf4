"""Sliding-window attention for the tests: with window W a row of length L attends slots [lo, L),
lo = max(0, L - W).  That is the un-windowed problem on the row's last min(L, W) tokens, so the references are the
existing ones applied to SLICES: per row, slots [lo, L) of K and V are moved to the front, the length becomes L - lo, and
heads_model.oracle_heads (the fp32 CPU oracle per head) and heads_model.HeadsModel (float64 per head) are applied
unchanged; with one head these are the plain oracle and the plain float64 model.  Errors, tolerance and the per-family
comparison are heads_model.compare's.

Score families are applied to the FULL row before slicing (accuracy_cases.apply_family sees the true lengths), so
`early_peak` puts its +30 tokens outside the window of every row longer than W + 16, and `flat` rows move by about 1 / W
for every token wrongly added or dropped.

TEST INFRASTRUCTURE, like heads_model.py and engine_sim.py: never used by the product."""
import numpy as np

import heads_model as hm
from accuracy_cases import edge_lengths
from engine_sim import CpuEngine
from helpers import PAGE

# (seed, B, S, D, heads, page types, windows, forced chunk_tokens, chunk sizes whose edges the lengths contain): the
# smallest shapes at which each mechanism of the windowed scan can still go wrong (tests/test_window_scan_gpu.py says which).
# fp8 pages exist with one head only.
WINDOW_SHAPES = [
    (401, 40, 64, 64, (1, 2), ("f32", "bf16", "fp8"), (1, 5, 16, 17, 33), (0,), (64,)),
    (402, 24, 256, 512, (1, 8), ("f32", "bf16", "fp8"), (40, 100, 255), (0, 256), (64,)),
    (403, 20, 1024, 256, (1, 2), ("f32", "bf16"), (100, 513), (0,), (64,)),
    (404, 24, 512, 1024, (1, 8), ("bf16", "fp8"), (130,), (0, 256), (64,)),
    (405, 8, 256, 2048, (1,), ("f32", "bf16", "fp8"), (100,), (0,), ()),
    (406, 700, 128, 64, (1, 2), ("f32",), (50,), (0,), (64,)),
    (407, 16, 4096, 512, (1, 4), ("bf16",), (1024,), (64, 1024), ()),
]


def window_lo(lengths, W):
    L = np.asarray(lengths).astype(np.int64)
    return np.maximum(L - int(W), 0)


def wanted_lengths(S, W, chunks):
    """The lengths every windowed case must contain: accuracy_cases.edge_lengths' edges with W among the chunk sizes, and
    W + 15, W + 16, W + 17 (with W + 1: a window that starts 15, 0 and 1 slots into a page), as far as they fit a row."""
    top = S - 1
    want = [0, 1, 2, 15, 16, 17, top - 1, top, W + 15, W + 16, W + 17]
    for c in tuple(chunks) + (W,):
        want += [c - 1, c, c + 1]
    return sorted({e for e in want if 0 <= e <= top})


def window_lengths(seed, B, S, W, chunks):
    """A list of length vectors for the case.  Normally one: accuracy_cases.edge_lengths with W among its chunk edges, the
    remaining wanted lengths written over its last (random) rows.  A batch with fewer rows than wanted lengths (B = 8) gets
    several vectors instead, each with 0 and S - 1 and its share of the rest."""
    want = wanted_lengths(S, W, chunks)
    forced = sorted({e for e in [0, 1, 2, 15, 16, 17, S - 2, S - 1] + [c + d for c in tuple(chunks) + (W,) for d in (-1, 0, 1)]
                     if 0 <= e <= S - 1})
    extra = [e for e in want if e not in forced]
    if B >= len(forced) + 2 + len(extra):
        L = edge_lengths(seed, B, S, tuple(chunks) + (W,))
        assert sorted(set(L[:len(forced)].tolist())) == forced
        if extra:
            L[B - len(extra):] = extra
        # a window close to n_sequence leaves few random rows as long as the window: make sure of six, so that a token
        # wrongly dropped from a `peaked` row is one that carries weight in at least one of them
        free = list(range(len(forced) + 2, B - len(extra)))
        rng = np.random.default_rng(seed + 9200)
        while (L >= W).sum() < 6 and free:
            L[free.pop()] = rng.integers(W, S)
        parts = [L]
    else:
        rest = [e for e in want if e not in (0, S - 1)]
        per = B - 2
        rng = np.random.default_rng(seed + 9100)
        parts = []
        for i in range(0, len(rest), per):
            share = rest[i:i + per]
            share += rng.integers(0, S, size=per - len(share)).tolist()
            parts.append(np.asarray([0] + share + [S - 1], np.int32))
    have = set(np.concatenate(parts).tolist())
    assert have >= set(want), sorted(set(want) - have)
    for L in parts:
        assert L.min() == 0 and L.max() == S - 1 and len(L) == B
    if S - 1 >= W + 17:
        assert {int(x) % PAGE for x in window_lo(np.concatenate(parts), W) if x > 0} >= {0, 1, 15}
    return parts


def low_dead_offsets(table, lengths, S, D, W):
    """Pool offsets (in elements) of the K and V segments of the slots below the window inside a row's first live page:
    16 * (lo // 16) <= s < lo (accuracy_cases.dead_slot_offsets is the same for the slots s >= L)."""
    lo = window_lo(lengths, W)
    s = np.arange(S)[None, :]
    b_idx, s_idx = np.nonzero((s >= (lo // PAGE * PAGE)[:, None]) & (s < lo[:, None]))
    page = table[b_idx, s_idx // PAGE]
    assert (page >= 0).all()
    off = page.astype(np.int64) + (s_idx % PAGE) * 3 * D + D
    return (off[:, None] + np.arange(2 * D)[None, :]).reshape(-1)


def compact(kt, v, lengths, mask):
    """(kt', v', L'): per row the slots s < L with mask[b, s] moved to the front in order, zeros behind them."""
    B, D, S = kt.shape
    kt2 = np.zeros((B, D, S), kt.dtype)
    v2 = np.zeros((B, S, D), v.dtype)
    L2 = np.zeros(B, np.int32)
    for b in range(B):
        idx = np.nonzero(mask[b, :int(lengths[b])])[0]
        n = len(idx)
        L2[b] = n
        if n:
            kt2[b, :, :n] = kt[b][:, idx]
            v2[b, :n] = v[b, idx]
    return kt2, v2, L2


def window_mask(lengths, S, W):
    s = np.arange(S)[None, :]
    L = np.asarray(lengths).astype(np.int64)[:, None]
    return (s >= np.maximum(L - int(W), 0)) & (s < L)


def window_slice(kt, v, lengths, W):
    """Slots [lo, L) of every row moved to the front; the new lengths are L - lo = min(L, W)."""
    return compact(kt, v, lengths, window_mask(lengths, kt.shape[2], W))


def oracle_window(oracle, q, kt, v, lengths, H, W):
    kt2, v2, L2 = window_slice(kt, v, lengths, W)
    return hm.oracle_heads(oracle, q, kt2, v2, L2, H)


def model_window(q, kt, v, lengths, H, W):
    kt2, v2, L2 = window_slice(kt, v, lengths, W)
    return hm.HeadsModel(q, kt2, v2, L2, H)


# ---- wrong models: the faults a windowed scan actually has, each as the set of slots it attends ----------------------------
def _range_mask(lengths, S, lo, hi):
    s = np.arange(S)[None, :]
    return (s >= np.maximum(lo, 0)[:, None]) & (s < np.maximum(hi, 0)[:, None])


def mask_window_ignored(lengths, S, W):
    L = np.asarray(lengths).astype(np.int64)
    return _range_mask(lengths, S, np.zeros_like(L), L)


def mask_lo_one_too_low(lengths, S, W):
    """W + 1 tokens"""
    L = np.asarray(lengths).astype(np.int64)
    return _range_mask(lengths, S, window_lo(L, W) - 1, L)


def mask_lo_one_too_high(lengths, S, W):
    """W - 1 tokens (of a row that has W or more)"""
    L = np.asarray(lengths).astype(np.int64)
    lo = window_lo(L, W)
    return _range_mask(lengths, S, np.where(L >= W, lo + 1, lo), L)


def mask_newest_excluded(lengths, S, W):
    """the window [lo - 1, L - 1)"""
    L = np.asarray(lengths).astype(np.int64)
    return _range_mask(lengths, S, window_lo(L, W) - 1, L - 1)


def mask_page_granular(lengths, S, W):
    """lo rounded down to a page start"""
    L = np.asarray(lengths).astype(np.int64)
    return _range_mask(lengths, S, window_lo(L, W) // PAGE * PAGE, L)


def mask_low_mask_on_every_page(lengths, S, W):
    """the first live page's low mask (slots t < lo % 16) applied to every page of the row"""
    L = np.asarray(lengths).astype(np.int64)
    lo = window_lo(L, W)
    s = np.arange(S)[None, :]
    return window_mask(lengths, S, W) & (s % PAGE >= (lo % PAGE)[:, None])


WRONG_MASKS = {"window ignored": mask_window_ignored, "lo one too low": mask_lo_one_too_low,
               "lo one too high": mask_lo_one_too_high, "newest token excluded": mask_newest_excluded,
               "page-granular window": mask_page_granular, "low mask on every page": mask_low_mask_on_every_page}


def wrong_model(name, q, kt, v, lengths, H, W):
    """(float64 attention [B, D] of the wrong model, whether it attends other slots than the window on any row)"""
    S = kt.shape[2]
    mask = WRONG_MASKS[name](lengths, S, W)
    L = np.asarray(lengths).astype(np.int64)[:, None]
    mask = mask & (np.arange(S)[None, :] < L)
    differs = bool((mask != window_mask(lengths, S, W)).any())
    kt2, v2, L2 = compact(kt, v, lengths, mask)
    return hm.HeadsModel(q, kt2, v2, L2, H).o, differs


# ---- the CPU engine with heads and a window ----------------------------------------------------------------------------------
class _WindowOracle(hm._HeadsOracle):
    """heads_model._HeadsOracle whose attention sees the newest `window` tokens of every row only."""

    def __init__(self, oracle, n_heads, window):
        super().__init__(oracle, n_heads)
        self._W = window

    def _attend(self, q, kt, v, lengths, att):
        att[...] = oracle_window(self._o, q, kt, v, lengths, self._H, self._W)


class WindowCpuEngine(CpuEngine):
    def __init__(self, oracle, model, items, n_batch, n_sequence, n_heads, window, bf16=False):
        self.window_oracle = _WindowOracle(oracle, n_heads, window)
        super().__init__(self.window_oracle, model, items, n_batch, n_sequence, bf16=bf16)


def run_window_cpu_engine(oracle, model, items, n_batch, n_sequence, n_heads, window, bf16=False):
    """({item id: all tokens}, smallest top-2 logit gap of the run)."""
    e = WindowCpuEngine(oracle, model, items, n_batch, n_sequence, n_heads, window, bf16=bf16)
    while not e.done():
        e.step()
    return e.finished, e.window_oracle.min_logit_gap
