"""ALiBi for the tests: a linear position bias per QUERY head on the multi-head paged scan.  For row b of length
L, query head h, K/V head h // g (g = H // Hkv) and an attended slot s

    x[h][s] = q_h . K_{h // g}[s] / sqrt(hd) + slopes[h] * (s - (L - 1))

with the attended set of gqa_model.model_gqa for the same (W, K): s < L and (s < K or s >= max(0, L - W)).  s is the ABSOLUTE
slot in the row.  Softmax and p . V are as there; with slopes all zero the model IS gqa_model.model_gqa
(tests/test_alibi_model_cpu.py holds that).

  AlibiModel   float64, with the per-(row, head) condition scale heads_model.heads_error divides by
  eval_fp32    the same expression in float32 numpy.  The tolerance of every comparison is f64_model.tolerance of ITS error under
               heads_model.heads_error (8 x its own worst error, floored at 16 * 2^-24): never from a kernel.
  WRONG        the faults a kernel with a position bias actually has, each as (slope of head h, position of slot s).  A constant
               shift per (row, head) is invisible to softmax, so a wrong FRAME is no fault; these are.
  AlibiSpec / audit   the engine replay audit (tests/replay_model.py, unchanged) with the bias in its forward: the rules are
               replay_model's -- E32 from a float32 forward over the same stored state, tol = 2 tol_logit, plus E_flip where the
               stored bits may differ.

TEST INFRASTRUCTURE, like gqa_model.py: never used by the product."""
import contextlib
import math
from dataclasses import dataclass

import numpy as np

import f64_model as fm
import heads_model as hm
import replay_model as rm
import sinks_model as sm
from helpers import PAGE


def standard_slopes(H):
    """An independent restatement of mli_alibi_slopes: the geometric series 2^(-8 / n), ... over the largest power of two
    n <= H, then the odd members of the series of 2 n."""
    n = 1 << (int(H).bit_length() - 1)
    first = [2.0 ** (-8.0 * (i + 1) / n) for i in range(n)]
    rest = [2.0 ** (-4.0 * (2 * k + 1) / n) for k in range(H - n)]
    return np.asarray(first + rest, np.float64).astype(np.float32)


def slope_sets(H, seed=0):
    """{name: slopes}: the standard ones, all negative (the bias grows with the distance: the mass moves to the oldest attended
    tokens), and mixed signs and magnitudes with a zero among them."""
    std = standard_slopes(H)
    rng = np.random.default_rng(7700 + seed + H)
    mixed = (std * rng.choice([-1.0, 1.0], size=H) * rng.uniform(0.25, 2.0, size=H)).astype(np.float32)
    mixed[H // 2] = 0.0
    if not (mixed > 0).any():
        mixed[0] = abs(mixed[0]) or np.float32(0.5)
    if not (mixed < 0).any():
        mixed[-1] = -abs(mixed[-1]) or np.float32(-0.5)
    return {"standard": std, "negative": (-std).astype(np.float32), "mixed": mixed}


def attended(lengths, S, W=0, K=0):
    """[B, S] bool: the attended set (W 0: no window)"""
    return sm.sink_mask(lengths, S, W if W and W > 0 else S, K)


def _positions(lengths, S, W, K, position):
    """[B, S] float64 positions of the slots by rule `position`, relative to the newest token where the rule is the right one"""
    L = np.asarray(lengths).astype(np.int64)[:, None]
    s = np.broadcast_to(np.arange(S, dtype=np.int64)[None, :], (len(lengths), S))
    if position == "absolute":
        return (s - (L - 1)).astype(np.float64)
    if position == "inside the page":
        return (s % PAGE).astype(np.float64)
    if position == "inside the item":
        return (s % 64).astype(np.float64)
    if position == "virtual row":
        Wm = W if W and W > 0 else S
        skip = sm.skipped_pages(np.asarray(lengths), Wm, K)[:, None]
        virt = np.where(s < PAGE * sm.sink_pages(K), s, s - PAGE * skip)
        return (virt - (L - PAGE * skip - 1)).astype(np.float64)
    raise ValueError(position)


def _evaluate(q, kt, v, lengths, H, Hkv, slopes, W, K, dtype, position="absolute", head_slope=None):
    """(o [B, D], o_scale [B, H]) with every operation in `dtype`; head_slope(h) = the index of the slope head h takes"""
    q, kt, v = (np.asarray(a).astype(dtype) for a in (q, kt, v))
    B, D = q.shape
    S = kt.shape[2]
    g, hd = H // Hkv, D // H
    mask = attended(lengths, S, W, K)
    some = mask.any(axis=1)
    pos = _positions(lengths, S, W, K, position).astype(dtype)
    inv = dtype(math.sqrt(hd))
    o = np.zeros((B, D), dtype)
    o_scale = np.zeros((B, H), np.float64)
    for h in range(H):
        qs, ks = hm.head_slice(h, H, D), hm.head_slice(h // g, H, D)
        m = dtype(np.asarray(slopes, np.float32)[h if head_slope is None else head_slope(h)])
        x = np.einsum("bd,bds->bs", q[:, qs], kt[:, ks, :]).astype(dtype) / inv + m * pos
        x = np.where(mask, x, dtype(-np.inf))
        top = np.where(some, x.max(axis=1), dtype(0))
        e = np.where(mask, np.exp(x - top[:, None]), dtype(0))        # exact zeros outside the attended set
        p = (e / np.where(some, e.sum(axis=1, dtype=dtype), dtype(1))[:, None]).astype(dtype)
        o[:, qs] = np.einsum("bs,bsd->bd", p, v[:, :, ks]).astype(dtype)
        o_scale[:, h] = np.einsum("bs,bsd->bd", p.astype(np.float64), np.abs(v[:, :, ks].astype(np.float64))).max(axis=1)
    return o, o_scale


class AlibiModel:
    """float64 attention with the bias and its condition scale per (row, head): what heads_model.heads_error takes"""

    def __init__(self, q, kt, v, lengths, H, Hkv, slopes, W=0, K=0):
        self.H, self.D = H, np.shape(q)[1]
        self.lengths = np.asarray(lengths).astype(np.int64)
        with np.errstate(invalid="ignore"):
            self.o, self.o_scale = _evaluate(np.nan_to_num(q), np.nan_to_num(kt), np.nan_to_num(v), lengths, H, Hkv, slopes, W, K,
                                             np.float64)


def eval_fp32(q, kt, v, lengths, H, Hkv, slopes, W=0, K=0):
    """the same expression in float32 numpy"""
    with np.errstate(invalid="ignore"):
        return _evaluate(np.nan_to_num(q), np.nan_to_num(kt), np.nan_to_num(v), lengths, H, Hkv, slopes, W, K, np.float32)[0]


def tolerance(model, o32):
    """f64_model.tolerance of the float32 evaluation's own error on these inputs"""
    return fm.tolerance(hm.heads_error(o32, model))


def compare(o, o32, model, what="", report=print):
    """(worst error of o, tolerance): reported before the caller asserts"""
    worst, e32 = float(hm.heads_error(o, model).max()), float(hm.heads_error(o32, model).max())
    tol = tolerance(model, o32)
    report(f"ALIBI {what}: got {worst:.3e}  fp32 numpy {e32:.3e}  tol {tol:.3e}")
    return worst, tol


# ---- wrong models ---------------------------------------------------------------------------------------------------------------
def lane_load_head(h, H, D, epl):
    """the head whose slope head h takes when the slope of a lane's FIRST unit serves both lane loads: unit u = lane + 64 j lies in
    head u // G (G = hd / epl lanes per head); the second load's units take the head of unit u - 64"""
    G = D // H // epl
    return h - 64 // G if h * G >= 64 else h


def wrong(name, q, kt, v, lengths, H, Hkv, slopes, W=0, K=0, epl=4):
    """float64 attention [B, D] of the wrong model"""
    g, D = H // Hkv, np.shape(q)[1]
    kw = {"slopes ignored": dict(slopes=np.zeros(H, np.float32)),
          "sign flipped": dict(slopes=-np.asarray(slopes)),
          "slope of head h + 1": dict(head_slope=lambda h: (h + 1) % H),
          "slope of the K/V head": dict(head_slope=lambda h: h // g),
          "position inside the page": dict(position="inside the page"),
          "position restarts at every item": dict(position="inside the item"),
          "gap under sinks not counted": dict(position="virtual row"),
          "first lane load's slope for both": dict(head_slope=lambda h: lane_load_head(h, H, D, epl))}[name]
    args = dict(slopes=slopes, position="absolute", head_slope=None)
    args.update(kw)
    return _evaluate(q, kt, v, lengths, H, Hkv, args["slopes"], W, K, np.float64, args["position"], args["head_slope"])[0]


WRONG = ("slopes ignored", "sign flipped", "slope of head h + 1", "slope of the K/V head", "position inside the page",
         "position restarts at every item", "gap under sinks not counted", "first lane load's slope for both")


# ---- the engine replay audit with the bias ----------------------------------------------------------------------------------------
@dataclass(frozen=True)
class AlibiSpec(rm.Spec):
    slopes: tuple = ()

    def name(self):
        return super().name() + " alibi"


def logits_from_state(x, K, V, wq, emb, mask, n_heads, slopes, rows, dtype=np.float64):
    """replay_model.logits_from_state with slopes[h] * (j - i) added to the scaled score of position j for the row of position i"""
    x, K, V, wq, emb = (np.asarray(a).astype(dtype) for a in (x, K, V, wq, emb))
    rows = np.asarray(rows)
    dist = (np.arange(K.shape[0])[None, :] - rows[:, None]).astype(dtype)
    x, mask = x[rows], mask[rows]
    D = x.shape[1]
    hd = D // n_heads
    q = x @ wq
    out = np.empty((x.shape[0], D), dtype)
    scale = dtype(1.0 / math.sqrt(hd))
    for h in range(n_heads):
        sl = slice(h * hd, (h + 1) * hd)
        s = np.where(mask, (q[:, sl] @ K[:, sl].T) * scale + dtype(np.float32(slopes[h])) * dist, dtype(-np.inf))
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p = p / p.sum(axis=1, keepdims=True, dtype=dtype)
        out[:, sl] = p @ V[:, sl]
    return out @ emb.T


class AlibiReplay(rm.Replay):
    def _logits(self, K, V, dtype=np.float64):
        return logits_from_state(self.x, K, V, self.wq, self.emb, self.mask, self.spec.n_heads, self.spec.slopes, self.rows, dtype)


@contextlib.contextmanager
def _alibi_forward():
    """replay_model's judges with AlibiReplay as their forward (the module itself is left as it is).  judge_item names its
    forward as the module global `Replay`, so that name is swapped for the duration of one audit: NOT safe beside another
    thread that audits through replay_model in the same process (pytest runs these tests in one thread, and the judge's cache
    is keyed by the spec, so an ALiBi result is never handed to a plain audit or the other way round)."""
    plain = rm.Replay
    rm.Replay = AlibiReplay
    try:
        yield
    finally:
        rm.Replay = plain


def audit(model, items, finished, spec, n_sequence, **kw):
    """replay_model.audit under an AlibiSpec"""
    assert isinstance(spec, AlibiSpec) and len(spec.slopes) == spec.n_heads
    with _alibi_forward():
        return rm.audit(model, items, finished, spec, n_sequence, **kw)


def generate(model, prompt, spec, n_sequence, wrong_slopes=None):
    """Decode one item greedily on the float64 ALiBi forward (the choice on the float32-rounded logits, as the CPU engines
    choose); wrong_slopes: the slopes the generator uses instead of the spec's (a wrong engine for the audit to reject)."""
    import sampling_ref as sr
    slopes = spec.slopes if wrong_slopes is None else wrong_slopes
    used = AlibiSpec(spec.store, spec.n_heads, spec.window, spec.n_sink, spec.flips, tuple(float(m) for m in slopes))
    toks = [int(t) for t in prompt]
    while True:
        rep = AlibiReplay(model, toks, used, rows=[len(toks) - 1])
        tok = int(sr.greedy(rep.logits[0].astype(np.float32)))
        toks.append(tok)
        if len(toks) >= n_sequence or tok == rm.EOF:
            return np.asarray(toks, np.int32)
