"""Learned attention-sink logits for the tests: one logit z_h per QUERY head on the multi-head paged scan and on the
causal prompt scan.  For row b of length L >= 1, query head h, K/V head h // g (g = H // Hkv), the attended set A of
gqa_model.model_gqa for the same (W, K) and the scaled scores x_s = q_h . K_{h // g}[s] / sqrt(hd)

    m     = max( max_{s in A} x_s , z_h )
    out_h = sum_{s in A} exp(x_s - m) V_{h // g}[s]  /  ( sum_{s in A} exp(x_s - m) + exp(z_h - m) )

z_h is one more logit of the head's softmax WITHOUT a value row; z_h = -inf is no sink, and then the model IS gqa_model.model_gqa
(tests/test_sink_logits_model_cpu.py holds that).  It is not the count K of sink TOKENS, which belongs to the attended set.

  SinkLogitsModel  float64, with the per-(row, head) condition scale heads_model.heads_error divides by (1 where the sink takes
                   the whole mass and the model's value is exactly 0) and the sink's softmax share per (row, head)
  eval_fp32        the same expression in float32 numpy.  The tolerance of every comparison is f64_model.tolerance of ITS error
                   under heads_model.heads_error (8 x its own worst error, floored at 16 * 2^-24): never from a kernel.
  WRONG            the faults a kernel with this switch actually has, each as a wrong model
  learned / mixed / none   the logit sets.  CONDITION: a sink far below a head's scores is invisible at fp32 accuracy whatever the
                   kernel does, so `learned` centres every head's logit on the median log-sum-exp of that head's scores over
                   the case's non-empty rows and `conditioned` holds the statement the comparisons rely on: on at least
                   MIN_BITING of the non-empty (row, head) pairs the sink's share lies in SHARE_BAND.
  prompt form      position t of a segment = the decode model on a virtual row of length t + 1 (prompt_model.virtual)
  SinkLogitsSpec / audit / generate   the engine replay audit (tests/replay_model.py, unchanged) with the sink in its forward

TEST INFRASTRUCTURE, like alibi_model.py and softcap_model.py: never used by the product."""
import contextlib
import math
from dataclasses import dataclass

import numpy as np

import f64_model as fm
import heads_model as hm
import replay_model as rm
import sinks_model as sm

FORMS = ((0, 0), (40, 0), (40, 4))
SHARE_BAND = (0.1, 0.9)     # the sink's softmax share under the float64 model at which a wrong sink is far above fp32 rounding
MIN_BITING = 0.5            # ... on at least this fraction of the non-empty (row, head) pairs of a case
FAR_ABOVE = 100.0           # "the maximum over the scores only" is judged at a logit this far above the largest score
ITEM_TOKENS = 64            # the smallest item of the chunked scan: "once per item" counts ceil(L / 64) sinks
# the logits of the engine tests (4 heads): large enough beside the scores of engine_sim.make_model(8648, ...) that the engine
# decodes other tokens than the plain one (tests/test_sink_logits_model_cpu.py holds that on the CPU)
ENGINE_LOGITS = (2.0, -1.0, 3.0, 0.5)


def attended(lengths, S, W=0, K=0):
    """[B, S] bool: the attended set (W 0: no window)"""
    return sm.sink_mask(lengths, S, W if W and W > 0 else S, K)


def second_lane_load(h, H, D, epl):
    """whether head h's lane units lie in the second lane load of a row: unit u = lane + 64 j lies in head u // G, G = hd / epl"""
    return h * (D // H // epl) >= 64


def _scores(q, kt, h, H, Hkv, dtype):
    D = q.shape[1]
    g, hd = H // Hkv, D // H
    raw = np.einsum("bd,bds->bs", q[:, hm.head_slice(h, H, D)], kt[:, hm.head_slice(h // g, H, D), :]).astype(dtype)
    return (raw / dtype(math.sqrt(hd))).astype(dtype)


def _evaluate(q, kt, v, lengths, H, Hkv, z, W, K, dtype, fault=None, epl=4):
    """(o [B, D], o_scale [B, H], share [B, H]) with every operation in `dtype`; fault: a name of WRONG or None"""
    q, kt, v = (np.asarray(a).astype(dtype) for a in (q, kt, v))
    z = np.asarray(z, np.float32).astype(dtype)
    L = np.asarray(lengths).astype(np.int64)
    B, D = q.shape
    S = kt.shape[2]
    g, hd = H // Hkv, D // H
    mask = attended(L, S, W, K)
    some = mask.any(axis=1)
    o = np.zeros((B, D), dtype)
    o_scale = np.zeros((B, H), np.float64)
    share = np.zeros((B, H), np.float64)
    for h in range(H):
        qs, ks = hm.head_slice(h, H, D), hm.head_slice(h // g, H, D)
        x = np.where(mask, _scores(q, kt, h, H, Hkv, dtype), dtype(-np.inf))
        zh = np.full(B, z[h], dtype)
        count = np.ones(B, dtype)                  # how often the sink enters the denominator
        in_max = True
        if fault == "sink ignored":
            zh[:] = -np.inf
        elif fault == "sink counted once per item":
            count = np.maximum(1, -(-mask.sum(axis=1) // ITEM_TOKENS)).astype(dtype)
        elif fault == "sink counted once per wave":
            count[:] = 4
        elif fault == "logit of the K/V head":
            zh[:] = z[h // g]
        elif fault == "logit of the neighbouring head":
            zh[:] = z[(h + 1) % H]
        elif fault == "logit divided by sqrt(head_dim)":
            zh = (zh / dtype(math.sqrt(hd))).astype(dtype)
        elif fault == "sink dropped where a window is active":
            zh = np.where((W > 0) & (L > W), dtype(-np.inf), zh)
        elif fault == "maximum over the scores only":
            in_max = False
        elif fault == "one lane load only":
            if second_lane_load(h, H, D, epl):
                zh[:] = -np.inf
        elif fault not in (None, "sink's mass on the newest token's V row"):
            raise ValueError(fault)
        top = x.max(axis=1)
        if in_max:
            top = np.maximum(top, zh)
        top = np.where(some, top, dtype(0))
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.where(mask, np.exp(x - top[:, None]), dtype(0))        # exact zeros outside the attended set
            ez = np.where(some, (count * np.exp(zh - top)).astype(dtype), dtype(0))
            denom = (e.sum(axis=1, dtype=dtype) + ez).astype(dtype)
            p = (e / np.where(some, denom, dtype(1))[:, None]).astype(dtype)
            pz = (ez / np.where(some, denom, dtype(1))).astype(dtype)
        vk = v[:, :, ks]
        o[:, qs] = np.einsum("bs,bsd->bd", p, vk).astype(dtype)
        if fault == "sink's mass on the newest token's V row":
            newest = vk[np.arange(B), np.maximum(L, 1) - 1]
            o[:, qs] += (pz[:, None] * newest).astype(dtype) * some[:, None]
        with np.errstate(invalid="ignore"):
            scale = np.einsum("bs,bsd->bd", np.nan_to_num(p.astype(np.float64)), np.abs(vk.astype(np.float64))).max(axis=1)
        o_scale[:, h] = np.where(scale > 0, scale, 1.0)
        share[:, h] = pz
    return o, o_scale, share


class SinkLogitsModel:
    """float64 attention with the sink logits, its condition scale and the sink's share per (row, head): what
    heads_model.heads_error takes"""

    def __init__(self, q, kt, v, lengths, H, Hkv, z, W=0, K=0):
        self.H, self.D = H, np.shape(q)[1]
        self.lengths = np.asarray(lengths).astype(np.int64)
        with np.errstate(invalid="ignore"):
            self.o, self.o_scale, self.share = _evaluate(np.nan_to_num(q), np.nan_to_num(kt), np.nan_to_num(v), lengths, H, Hkv, z,
                                                         W, K, np.float64)


def eval_fp32(q, kt, v, lengths, H, Hkv, z, W=0, K=0):
    """the same expression in float32 numpy"""
    with np.errstate(invalid="ignore"):
        return _evaluate(np.nan_to_num(q), np.nan_to_num(kt), np.nan_to_num(v), lengths, H, Hkv, z, W, K, np.float32)[0]


def tolerance(model, o32):
    """f64_model.tolerance of the float32 evaluation's own error on these inputs"""
    return fm.tolerance(hm.heads_error(o32, model))


def compare(o, o32, model, what="", report=print):
    """(worst error of o, tolerance): reported before the caller asserts"""
    worst, e32 = float(hm.heads_error(o, model).max()), float(hm.heads_error(o32, model).max())
    tol = tolerance(model, o32)
    report(f"SINK_LOGITS {what}: got {worst:.3e}  fp32 numpy {e32:.3e}  tol {tol:.3e}  got/tol {worst / tol:.3f}")
    return worst, tol


WRONG = ("sink ignored", "sink counted once per item", "sink counted once per wave", "logit of the K/V head",
         "logit of the neighbouring head", "logit divided by sqrt(head_dim)", "sink dropped where a window is active",
         "sink's mass on the newest token's V row", "maximum over the scores only", "one lane load only")


def wrong(name, q, kt, v, lengths, H, Hkv, z, W=0, K=0, epl=4):
    """attention [B, D] of the wrong model, float64 -- except "maximum over the scores only", whose fault IS float32's range
    (exp of a large positive difference): that one is evaluated in float32 and returned as float64"""
    assert name in WRONG
    dtype = np.float32 if name == "maximum over the scores only" else np.float64
    with np.errstate(invalid="ignore", over="ignore"):
        return _evaluate(np.nan_to_num(q), np.nan_to_num(kt), np.nan_to_num(v), lengths, H, Hkv, z, W, K, dtype, name,
                         epl)[0].astype(np.float64)


# ---- the logit sets and the condition on them -------------------------------------------------------------------------------------
def log_sum_exp(q, kt, lengths, H, Hkv, W=0, K=0):
    """[B, H] float64: log sum_{s in A} exp(x_s) per (row, head); -inf for an empty row"""
    q, kt = np.nan_to_num(np.asarray(q, np.float64)), np.nan_to_num(np.asarray(kt, np.float64))
    mask = attended(lengths, kt.shape[2], W, K)
    out = np.full((q.shape[0], H), -np.inf)
    rows = mask.any(axis=1)
    for h in range(H):
        x = np.where(mask, _scores(q, kt, h, H, Hkv, np.float64), -np.inf)[rows]
        top = x.max(axis=1)
        out[rows, h] = top + np.log(np.exp(x - top[:, None]).sum(axis=1))
    return out


def largest_score(q, kt, lengths, H, Hkv, W=0, K=0):
    q, kt = np.nan_to_num(np.asarray(q, np.float64)), np.nan_to_num(np.asarray(kt, np.float64))
    mask = attended(lengths, kt.shape[2], W, K)
    return max(float(np.where(mask, _scores(q, kt, h, H, Hkv, np.float64), -np.inf).max()) for h in range(H))


def head_offsets(H):
    """LEARNED's offset per head: in [-1, 1], of alternating sign, different from head to head"""
    return np.linspace(-1.0, 1.0, H) * np.where(np.arange(H) % 2 == 0, 1.0, -1.0)


def learned(q, kt, lengths, H, Hkv, W=0, K=0):
    """LEARNED for a case: finite float32 logits spread over the heads -- head h's logit is the median log-sum-exp of head h's
    scores over the non-empty rows plus an offset in [-1, 1] that differs from head to head (the share of a sink at the
    log-sum-exp itself is 1/2)."""
    lse = log_sum_exp(q, kt, lengths, H, Hkv, W, K)
    rows = np.isfinite(lse[:, 0])
    centre = np.median(lse[rows], axis=0) if rows.any() else np.zeros(H)
    return (centre + head_offsets(H)).astype(np.float32)


def none(H):
    """NONE: no sink in any head"""
    return np.full(H, -np.inf, np.float32)


def mixed(z):
    """MIXED: LEARNED with one head at -inf, one at -1e30 and one at +1e30.  With four heads or more that is one vector (the
    +1e30 in the last head: the second lane load where a row has two); with fewer, two vectors that hold the three between them.
    Returns [(logits, {kind: head})]."""
    z = np.asarray(z, np.float32)
    H = len(z)
    if H >= 4:
        a = z.copy()
        a[0], a[1], a[H - 1] = -np.inf, -1e30, 1e30
        return [(a, {"-inf": 0, "-1e30": 1, "+1e30": H - 1})]
    a, b = z.copy(), z.copy()
    a[0], a[H - 1] = -np.inf, 1e30
    b[0] = -1e30
    return [(a, {"-inf": 0, "+1e30": H - 1}), (b, {"-1e30": 0})]


def biting_fraction(model):
    """the fraction of the non-empty (row, head) pairs on which the sink's share lies in SHARE_BAND"""
    rows = model.lengths > 0
    if not rows.any():
        return 1.0
    s = model.share[rows]
    return float(((s >= SHARE_BAND[0]) & (s <= SHARE_BAND[1])).mean())


def conditioned(model, what=""):
    """assert the condition under which a comparison against `model` bites"""
    f = biting_fraction(model)
    assert f >= MIN_BITING, f"{what}: the sink's share lies in {SHARE_BAND} on {f:.2f} of the non-empty (row, head) pairs only"
    return f


def rounded(a, elem):
    """the float32 values a page of type `elem` holds for the float32 array a ("bf16": round to nearest even)"""
    if elem == "f32":
        return np.asarray(a, np.float32)
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


# ---- the independent check: the sink as one crafted token ------------------------------------------------------------------------
def crafted_token(q, H, Hkv, z):
    """(K row [B, D], V row [B, D]) of a token that scores z_h against q_h for every query head h WITHOUT grouping
    (Hkv == H): K_h = z_h sqrt(hd) q_h / |q_h|^2, V = 0.  A row lengthened by this token is the row with the sink."""
    assert H == Hkv, "one K row cannot score differently against the heads of a group"
    q = np.asarray(q, np.float64)
    B, D = q.shape
    hd = D // H
    k = np.zeros((B, D))
    for h in range(H):
        sl = hm.head_slice(h, H, D)
        n2 = np.maximum((q[:, sl] ** 2).sum(axis=1), 1e-30)
        k[:, sl] = float(z[h]) * math.sqrt(hd) * q[:, sl] / n2[:, None]
    return k.astype(np.float32), np.zeros((B, D), np.float32)


# ---- the prompt form ---------------------------------------------------------------------------------------------------------------
def prompt_model(qv, kt, v, rows, pos, H, Hkv, z, W=0, K=0):
    """SinkLogitsModel over the virtual rows of the queries: query i = its own q, the K and V of its row, length pos + 1"""
    import prompt_model as pm
    ktv, vv, Lv = pm.virtual(kt, v, rows, pos)
    return SinkLogitsModel(qv, ktv, vv, Lv, H, Hkv, z, W, K)


def prompt_eval_fp32(qv, kt, v, rows, pos, H, Hkv, z, W=0, K=0):
    import prompt_model as pm
    ktv, vv, Lv = pm.virtual(kt, v, rows, pos)
    return eval_fp32(qv, ktv, vv, Lv, H, Hkv, z, W, K)


# ---- the engine replay audit with the sink logits ---------------------------------------------------------------------------------
@dataclass(frozen=True)
class SinkLogitsSpec(rm.Spec):
    logits: tuple = ()        # one per head; (): none (the plain forward)

    def name(self):
        return super().name() + " sink logits"


def logits_from_state(x, K, V, wq, emb, mask, n_heads, z, rows, dtype=np.float64, rope_table=None):
    """replay_model.logits_from_state with z[h] as one more logit of head h's softmax without a value row (z empty: none);
    rope_table given: q of position i rotated by table[i] as rope_model.logits_from_state rotates it"""
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
        s = np.where(mask, ((q[:, sl] @ K[:, sl].T) * scale).astype(dtype), dtype(-np.inf))
        zh = dtype(np.float32(z[h])) if len(z) else dtype(-np.inf)
        top = np.maximum(s.max(axis=1, keepdims=True), zh)
        p = np.exp(s - top)
        p = p / (p.sum(axis=1, keepdims=True, dtype=dtype) + np.exp(zh - top)).astype(dtype)
        out[:, sl] = p @ V[:, sl]
    return out @ emb.T


class SinkLogitsReplay(rm.Replay):
    def _logits(self, K, V, dtype=np.float64):
        return logits_from_state(self.x, K, V, self.wq, self.emb, self.mask, self.spec.n_heads, self.spec.logits, self.rows, dtype)


@contextlib.contextmanager
def sink_forward(replay=SinkLogitsReplay):
    """replay_model's judges (and prompt_model.prompt_replay) with SinkLogitsReplay as their forward; the module itself is left as
    it is.  As alibi_model._alibi_forward: the module global `Replay` is swapped for the duration of one audit, NOT safe beside
    another thread that audits through replay_model in the same process; the judge's cache is keyed by the spec."""
    plain = rm.Replay
    rm.Replay = replay
    try:
        yield
    finally:
        rm.Replay = plain


def audit(model, items, finished, spec, n_sequence, **kw):
    """replay_model.audit under a SinkLogitsSpec"""
    assert isinstance(spec, SinkLogitsSpec) and len(spec.logits) == spec.n_heads
    with sink_forward():
        return rm.audit(model, items, finished, spec, n_sequence, **kw)


def generate(model, prompt, spec, n_sequence, wrong_logits=None):
    """Decode one item greedily on the float64 forward with the sink logits (the choice on the float32-rounded logits, as the CPU
    engines choose); wrong_logits: the logits the generator uses instead of the spec's (()): none) -- a wrong engine for the
    audit to reject."""
    import sampling_ref as sr
    z = spec.logits if wrong_logits is None else wrong_logits
    used = SinkLogitsSpec(spec.store, spec.n_heads, spec.window, spec.n_sink, spec.flips, tuple(float(t) for t in z))
    toks = [int(t) for t in prompt]
    while True:
        rep = SinkLogitsReplay(model, toks, used, rows=[len(toks) - 1])
        tok = int(sr.greedy(rep.logits[0].astype(np.float32)))
        toks.append(tok)
        if len(toks) >= n_sequence or tok == rm.EOF:
            return np.asarray(toks, np.int32)


def rope_audit(model, items, finished, spec, table, n_sequence, **kw):
    """replay_model.audit of an engine with a rotary table AND sink logits: rope_model.RopeReplay's stored state (K rotated before
    its one rounding) with the sink in the softmax of the rotated q.  spec: a SinkLogitsSpec; table: float32 [S, hd / 2, 2]."""
    import rope_model as rp

    @dataclass(frozen=True)
    class RopeSinkLogitsSpec(rp.RopeSpec):
        logits: tuple = ()

        def name(self):
            return super().name() + " sink logits"

    class RopeSinkLogitsReplay(rp.RopeReplay):
        def _logits(self, K, V, dtype=np.float64):
            return logits_from_state(self.x, K, V, self.wq, self.emb, self.mask, self.spec.n_heads, self.spec.logits, self.rows,
                                     dtype, rope_table=self.table)

    assert isinstance(spec, SinkLogitsSpec) and len(spec.logits) == spec.n_heads
    both = RopeSinkLogitsSpec(spec.store, spec.n_heads, spec.window, spec.n_sink, spec.flips,
                              np.ascontiguousarray(table, np.float32).tobytes(), tuple(spec.logits))
    with sink_forward(RopeSinkLogitsReplay):
        return rm.audit(model, items, finished, both, n_sequence, **kw)


# ---- the cases of tests/test_sink_logits_scan_gpu.py, built without a GPU ----------------------------------------------------------
# (seed, B, S, D, ((H, Hkv), ...), page types, chunk_tokens settings): the smallest shapes at which each mechanism can go wrong
SCAN_SHAPES = (
    (811, 40, 64, 64, ((2, 2), (2, 1)), ("f32", "bf16"), (0,)),            # one workgroup per row; dead lanes
    (812, 24, 256, 512, ((8, 8), (8, 2), (2, 2)), ("f32", "bf16"), (0, 256)),   # several items per row; f32: two lane loads
    (813, 20, 1024, 256, ((8, 2),), ("bf16",), (64,)),                     # 16 items per row; the query head's logit in a group
    (814, 700, 128, 64, ((2, 2),), ("f32",), (0,)),                        # rows handed out longest first
)
SCAN_CASES = tuple((seed, B, S, D, H, Hkv, elem, chunks) for seed, B, S, D, heads, elems, chunks in SCAN_SHAPES
                   for elem in elems for H, Hkv in heads)


def scan_lengths(seed, B, S):
    """accuracy_cases.edge_lengths: 0, 1, 2, 15, 16, 17, chunk +- 1, S - 1 in the first rows, random rows behind them"""
    from accuracy_cases import edge_lengths
    return edge_lengths(seed, B, S, tuple(c for c in (64, 256) if c < S))


_CASE_CACHE = {}


def scan_case(seed, B, S, D):
    """(case dict, fp32 pool, dead-slot offsets, lengths) of a scan shape: computed once and left unchanged"""
    key = (seed, B, S, D)
    if key not in _CASE_CACHE:
        import oracle
        from accuracy_cases import base_case, fill_pages
        oracle.lib()
        L = scan_lengths(seed, B, S)
        c = base_case(seed, B, S, D, L)
        pool32, dead = fill_pages(oracle, c, c["q_output"], c["kt_cache"], c["v_cache"])
        _CASE_CACHE.clear()          # one case at a time: the pools are large
        _CASE_CACHE[key] = (c, pool32, dead, L)
    return _CASE_CACHE[key]


def scan_operands(seed, B, S, D, elem, values=None):
    """(q [B, D], kt [B, D, S'], v [B, S', D], L): what the pages of type `elem` hold for the case, float32 values; `values`: the
    pool's values where the caller has them from the device already"""
    c, pool32, _, L = scan_case(seed, B, S, D)
    vals = rounded(pool32, elem) if values is None else values
    s_live = max(-(-int(L.max()) // 16) * 16, 16)
    kt = fm.gather_pages(vals, c["table"], L, s_live, D, 1).transpose(0, 2, 1)
    v = fm.gather_pages(vals, c["table"], L, s_live, D, 2)
    return c["q_output"], kt, v, L
