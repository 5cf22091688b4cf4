"""Attention logit soft-capping for the tests: one cap > 0 per call on the multi-head paged scan and on the causal
prompt scan.  For row b of length L, query head h, K/V head h // g (g = H // Hkv) and an attended slot s

    x[h][s] = cap * tanh( (q_h . K_{h // g}[s] / sqrt(hd)) / cap )

with the attended set of gqa_model.model_gqa for the same (W, K): s < L and (s < K or s >= max(0, L - W)).  Softmax and p . V are
as there.  There is no cap that gives back the uncapped model.

  SoftcapModel  float64, gqa_model.model_gqa's structure with the cap, and the per-(row, head) condition scale
                heads_model.heads_error divides by
  eval_fp32     the same expression in float32 numpy: x / cap, np.tanh and the product each rounded to float32.  The tolerance of
                every comparison is f64_model.tolerance of ITS error under heads_model.heads_error (8 x its own worst error,
                floored at 16 * 2^-24): never from a kernel.
  prompt form   position t of a segment = the decode model on a virtual row of length t + 1 (prompt_model.virtual)
  WRONG         the faults a kernel with a cap actually has, each as a wrong model
  scale_q       the condition on the INPUTS under which the comparison bites: q scaled so that the largest attended |score|
                is a given value (the tests take half the largest cap).  A cap far above every score is invisible at fp32
                accuracy whatever the kernel does; tests/test_softcap_model_cpu.py holds the margin on the CPU.
  SoftcapSpec / audit / generate   the engine replay audit (tests/replay_model.py, unchanged) with the cap in its forward

TEST INFRASTRUCTURE, like alibi_model.py: never used by the product."""
import contextlib
import math
from dataclasses import dataclass

import numpy as np

import f64_model as fm
import heads_model as hm
import replay_model as rm
import sinks_model as sm

CAPS = (50.0, 5.0, 1.0)
# the cap of the engine tests: small enough beside the scores of engine_sim.make_model(8648, ...) that the capped engine decodes
# other tokens than the plain one (tests/test_softcap_model_cpu.py holds that on the CPU)
ENGINE_CAP = 2.0
FORMS = ((0, 0), (40, 0), (5, 0), (40, 4), (40, 20))


def attended(lengths, S, W=0, K=0):
    """[B, S] bool: the attended set (W 0: no window)"""
    return sm.sink_mask(lengths, S, W if W and W > 0 else S, K)


def second_lane_load(h, H, D, epl):
    """whether head h's lane units lie in the second lane load of a row: unit u = lane + 64 j lies in head u // G, G = hd / epl"""
    return h * (D // H // epl) >= 64


def _capped(x, cap, dtype):
    return (dtype(cap) * np.tanh((x / dtype(cap)).astype(dtype)).astype(dtype)).astype(dtype)


def _evaluate(q, kt, v, lengths, H, Hkv, cap, W, K, dtype, fault=None, epl=4):
    """(o [B, D], o_scale [B, H]) with every operation in `dtype`; fault: a name of WRONG or None"""
    q, kt, v = (np.asarray(a).astype(dtype) for a in (q, kt, v))
    B, D = q.shape
    S = kt.shape[2]
    g, hd = H // Hkv, D // H
    mask = attended(lengths, S, W, K)
    inv = dtype(math.sqrt(hd))
    c = dtype(cap)
    o = np.zeros((B, D), dtype)
    o_scale = np.zeros((B, H), np.float64)
    for h in range(H):
        qs, ks = hm.head_slice(h, H, D), hm.head_slice(h // g, H, D)
        raw = np.einsum("bd,bds->bs", q[:, qs], kt[:, ks, :]).astype(dtype)
        x = (raw / inv).astype(dtype)
        live = mask
        if fault is None:
            x = _capped(x, cap, dtype)
        elif fault == "cap ignored":
            pass
        elif fault == "cap before the scaling":
            x = (_capped(raw, cap, dtype) / inv).astype(dtype)
        elif fault == "cap * tanh(x) without the division":
            x = c * np.tanh(x)
        elif fault == "tanh(x / cap) without the multiplication":
            x = np.tanh(x / c)
        elif fault == "hard clip at +-cap":
            x = np.clip(x, -c, c)
        elif fault == "cap after the maximum is subtracted":
            top = np.where(mask, x, -np.inf).max(axis=1, initial=-np.inf)
            x = _capped(x - np.where(np.isfinite(top), top, 0)[:, None], cap, dtype)
        elif fault == "masked slots admitted at -cap":       # tanh(-inf) = -1: every slot of a non-empty row takes part
            x = np.where(mask, _capped(x, cap, dtype), -c)
            live = np.broadcast_to(mask.any(axis=1)[:, None], mask.shape)
        elif fault == "one lane load only":
            x = x if second_lane_load(h, H, D, epl) else _capped(x, cap, dtype)
        else:
            raise ValueError(fault)
        some = live.any(axis=1)
        x = np.where(live, x, dtype(-np.inf))
        top = np.where(some, x.max(axis=1), dtype(0))
        e = np.where(live, np.exp(x - top[:, None]), dtype(0))        # exact zeros outside the attended set
        p = (e / np.where(some, e.sum(axis=1, dtype=dtype), dtype(1))[:, None]).astype(dtype)
        o[:, qs] = np.einsum("bs,bsd->bd", p, v[:, :, ks]).astype(dtype)
        o_scale[:, h] = np.einsum("bs,bsd->bd", p.astype(np.float64), np.abs(v[:, :, ks].astype(np.float64))).max(axis=1)
    return o, o_scale


class SoftcapModel:
    """float64 attention with the cap and its condition scale per (row, head): what heads_model.heads_error takes"""

    def __init__(self, q, kt, v, lengths, H, Hkv, cap, W=0, K=0):
        self.H, self.D = H, np.shape(q)[1]
        self.lengths = np.asarray(lengths).astype(np.int64)
        with np.errstate(invalid="ignore"):
            self.o, self.o_scale = _evaluate(np.nan_to_num(q), np.nan_to_num(kt), np.nan_to_num(v), lengths, H, Hkv, cap, W, K,
                                             np.float64)


def eval_fp32(q, kt, v, lengths, H, Hkv, cap, W=0, K=0):
    """the same expression in float32 numpy"""
    with np.errstate(invalid="ignore"):
        return _evaluate(np.nan_to_num(q), np.nan_to_num(kt), np.nan_to_num(v), lengths, H, Hkv, cap, W, K, np.float32)[0]


def tolerance(model, o32):
    """f64_model.tolerance of the float32 evaluation's own error on these inputs"""
    return fm.tolerance(hm.heads_error(o32, model))


def compare(o, o32, model, what="", report=print):
    """(worst error of o, tolerance): reported before the caller asserts"""
    worst, e32 = float(hm.heads_error(o, model).max()), float(hm.heads_error(o32, model).max())
    tol = tolerance(model, o32)
    report(f"SOFTCAP {what}: got {worst:.3e}  fp32 numpy {e32:.3e}  tol {tol:.3e}  got/tol {worst / tol:.3f}")
    return worst, tol


WRONG = ("cap ignored", "cap before the scaling", "cap * tanh(x) without the division", "tanh(x / cap) without the multiplication",
         "hard clip at +-cap", "cap after the maximum is subtracted", "masked slots admitted at -cap", "one lane load only")


def wrong(name, q, kt, v, lengths, H, Hkv, cap, W=0, K=0, epl=4):
    """float64 attention [B, D] of the wrong model"""
    assert name in WRONG
    with np.errstate(invalid="ignore"):
        return _evaluate(np.nan_to_num(q), np.nan_to_num(kt), np.nan_to_num(v), lengths, H, Hkv, cap, W, K, np.float64, name, epl)[0]


# ---- the condition on the inputs ---------------------------------------------------------------------------------------------------
def largest_score(q, kt, lengths, H, Hkv):
    """the largest |q_h . K_{h // g}[s] / sqrt(hd)| over the slots s < L of every row and head, float64"""
    q, kt = np.nan_to_num(np.asarray(q, np.float64)), np.nan_to_num(np.asarray(kt, np.float64))
    B, D = q.shape
    g, hd = H // Hkv, D // H
    mask = attended(lengths, kt.shape[2])
    worst = 0.0
    for h in range(H):
        x = np.einsum("bd,bds->bs", q[:, hm.head_slice(h, H, D)], kt[:, hm.head_slice(h // g, H, D), :]) / math.sqrt(hd)
        worst = max(worst, float(np.abs(np.where(mask, x, 0.0)).max()))
    return worst


def scale_q(q, kt, lengths, H, Hkv, target=CAPS[0] / 2):
    """q (float32) scaled so that largest_score is `target`: some scores reach half the largest cap, most lie far below it"""
    top = largest_score(q, kt, lengths, H, Hkv)
    return (np.asarray(q, np.float32) * np.float32(target / top)).astype(np.float32) if top > 0 else np.asarray(q, np.float32)


def repelled_case(q, kt, lengths, H, Hkv, depth=2.0 * CAPS[0], seed=0):
    """(q, kt) on which every attended score is NEGATIVE, between about -depth and -0.8 depth: K's columns are -q of their query
    group's first head times a factor in [0.8, 1].  The inputs on which a masked slot admitted at -cap shows at the largest cap:
    the live scores saturate near -cap themselves, so a dead slot at -cap weighs as much as a live one.  (Under grouping the
    other heads of a group see mixed signs; the first head of each group carries the comparison.)"""
    q = np.nan_to_num(np.asarray(q, np.float32)).copy()
    B, D = q.shape
    S = np.shape(kt)[2]
    g, hd = H // Hkv, D // H
    rng = np.random.default_rng(9900 + seed)
    out = np.zeros((B, D, S), np.float32)
    for kv in range(Hkv):
        qh = q[:, hm.head_slice(kv * g, H, D)].astype(np.float64)
        n2 = np.maximum((qh * qh).sum(axis=1), 1e-30)
        f = rng.uniform(0.8, 1.0, size=(B, 1, S))
        out[:, hm.head_slice(kv, H, D), :] = (-depth * math.sqrt(hd) * qh / n2[:, None])[:, :, None] * f
    return q, out


# ---- the prompt form ---------------------------------------------------------------------------------------------------------------
def prompt_model(qv, kt, v, rows, pos, H, Hkv, cap, W=0, K=0):
    """SoftcapModel over the virtual rows of the queries: query i = its own q, the K and V of its row, length pos + 1"""
    import prompt_model as pm
    ktv, vv, Lv = pm.virtual(kt, v, rows, pos)
    return SoftcapModel(qv, ktv, vv, Lv, H, Hkv, cap, W, K)


def prompt_eval_fp32(qv, kt, v, rows, pos, H, Hkv, cap, W=0, K=0):
    import prompt_model as pm
    ktv, vv, Lv = pm.virtual(kt, v, rows, pos)
    return eval_fp32(qv, ktv, vv, Lv, H, Hkv, cap, W, K)


# ---- the engine replay audit with the cap ------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SoftcapSpec(rm.Spec):
    cap: float = 0.0          # 0: no cap (the plain forward)

    def name(self):
        return super().name() + f" softcap {self.cap:g}"


def logits_from_state(x, K, V, wq, emb, mask, n_heads, cap, rows, dtype=np.float64, rope_table=None):
    """replay_model.logits_from_state with cap * tanh(score / cap) on the scaled scores (cap 0: none); rope_table given: q of
    position i rotated by table[i] as rope_model.logits_from_state rotates it (K arrives rotated by its slot)"""
    x, K, V, wq, emb = (np.asarray(a).astype(dtype) for a in (x, K, V, wq, emb))
    rows = np.asarray(rows)
    x, mask = x[rows], mask[rows]
    D = x.shape[1]
    hd = D // n_heads
    q = x @ wq
    if rope_table is not None:
        import rope_model as rp
        q = rp.rotate(q, rows, rope_table, n_heads, dtype=dtype).astype(dtype)
    out = np.empty((x.shape[0], D), dtype)
    scale = dtype(1.0 / math.sqrt(hd))
    for h in range(n_heads):
        sl = slice(h * hd, (h + 1) * hd)
        s = ((q[:, sl] @ K[:, sl].T) * scale).astype(dtype)
        if cap:
            s = _capped(s, cap, dtype)
        s = np.where(mask, s, dtype(-np.inf))
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p = p / p.sum(axis=1, keepdims=True, dtype=dtype)
        out[:, sl] = p @ V[:, sl]
    return out @ emb.T


class SoftcapReplay(rm.Replay):
    def _logits(self, K, V, dtype=np.float64):
        return logits_from_state(self.x, K, V, self.wq, self.emb, self.mask, self.spec.n_heads, self.spec.cap, self.rows, dtype)


@contextlib.contextmanager
def capped_forward():
    """replay_model's judges (and prompt_model.prompt_replay) with SoftcapReplay as their forward; the module itself is left as
    it is.  As alibi_model._alibi_forward: the module global `Replay` is swapped for the duration of one audit, NOT safe beside
    another thread that audits through replay_model in the same process; the judge's cache is keyed by the spec."""
    plain = rm.Replay
    rm.Replay = SoftcapReplay
    try:
        yield
    finally:
        rm.Replay = plain


def audit(model, items, finished, spec, n_sequence, **kw):
    """replay_model.audit under a SoftcapSpec"""
    assert isinstance(spec, SoftcapSpec) and spec.cap > 0
    with capped_forward():
        return rm.audit(model, items, finished, spec, n_sequence, **kw)


def generate(model, prompt, spec, n_sequence, wrong_cap=None):
    """Decode one item greedily on the float64 capped forward (the choice on the float32-rounded logits, as the CPU engines
    choose); wrong_cap: the cap the generator uses instead of the spec's (0: none) -- a wrong engine for the audit to reject."""
    import sampling_ref as sr
    cap = spec.cap if wrong_cap is None else wrong_cap
    used = SoftcapSpec(spec.store, spec.n_heads, spec.window, spec.n_sink, spec.flips, float(cap))
    toks = [int(t) for t in prompt]
    while True:
        rep = SoftcapReplay(model, toks, used, rows=[len(toks) - 1])
        tok = int(sr.greedy(rep.logits[0].astype(np.float32)))
        toks.append(tok)
        if len(toks) >= n_sequence or tok == rm.EOF:
            return np.asarray(toks, np.int32)


# ---- ... and beside rotary position embeddings (Gemma 2 uses both) ----------------------------------------------------------------
def rope_audit(model, items, finished, spec, table, n_sequence, **kw):
    """replay_model.audit of an engine with a rotary table AND a cap: rope_model.RopeReplay's stored state (K rotated before
    its one rounding) with the cap on the scores of the rotated q.  spec: a SoftcapSpec; table: float32 [S, hd / 2, 2]."""
    import rope_model as rp

    @dataclass(frozen=True)
    class RopeSoftcapSpec(rp.RopeSpec):
        cap: float = 0.0

        def name(self):
            return super().name() + f" softcap {self.cap:g}"

    class RopeSoftcapReplay(rp.RopeReplay):
        def _logits(self, K, V, dtype=np.float64):
            return logits_from_state(self.x, K, V, self.wq, self.emb, self.mask, self.spec.n_heads, self.spec.cap, self.rows, dtype,
                                     rope_table=self.table)

    assert isinstance(spec, SoftcapSpec) and spec.cap > 0
    both = RopeSoftcapSpec(spec.store, spec.n_heads, spec.window, spec.n_sink, spec.flips,
                           np.ascontiguousarray(table, np.float32).tobytes(), float(spec.cap))
    plain = rm.Replay
    rm.Replay = RopeSoftcapReplay
    try:
        return rm.audit(model, items, finished, both, n_sequence, **kw)
    finally:
        rm.Replay = plain
