"""Multi-head attention for the tests: n_heads = H heads of head_dim hd = D / H, head h owning columns
[h * hd, (h + 1) * hd) of q, K and V, are H independent single-head problems of width hd.  So the references are the
existing ones applied to contiguous slices: the fp32 CPU oracle's three stages (accuracy_cases.oracle_scan, which then
divides by sqrt(hd)) and the float64 model (f64_model.scores / softmax / attend / attend_abs).

Errors are per (row, head): max_d |o - o^| / max_d sum_s p^_s |v_sd| over the head's columns; a row of length 0 must be
exactly 0; a non-finite value is an infinite error.  The tolerance is the project's rule (f64_model.tolerance) from the
oracle's own error on the same inputs, taken separately per score family: the +-200 families carry ~2e-5 of
cancellation and would otherwise hide a last-digit error on a flat head.

Score families are applied per head (accuracy_cases.apply_family on the head's slice), by one of three assignments:
  mixed    head h gets MIXED[h % 6]: the heads of a row differ
  offsets  offset+ on even heads, offset- on odd ones: a running maximum or a probability shared between neighbouring
           heads gives exp(-400) = 0 and then 0 / 0
  flat     every head flat: p ~ 1 / L, the tolerance at its floor of a few ulp

TEST INFRASTRUCTURE, like engine_sim.py: never used by the product."""
import math

import numpy as np

import f64_model as fm
from accuracy_cases import apply_family, oracle_scan
from engine_sim import CpuEngine

MIXED = ("peaked", "offset+", "late_peak", "flat", "offset-", "early_peak")
ASSIGNMENTS = ("mixed", "offsets", "flat")

# (seed, B, S, D, heads, page types, chunk sizes whose edges the lengths contain): the smallest shapes at which each
# mechanism of the multi-head scan can still go wrong (tests/test_heads_scan_gpu.py says which)
HEAD_SHAPES = [
    (301, 40, 64, 64, (2,), ("f32", "bf16"), (64,)),
    (302, 24, 256, 512, (8, 2), ("f32", "bf16"), (64, 256)),
    (303, 24, 256, 192, (3,), ("f32", "bf16"), (64, 256)),
    (304, 20, 1024, 256, (2, 8), ("f32", "bf16"), (64, 256)),
    (305, 24, 512, 1024, (8,), ("bf16",), (64, 256)),
    (306, 16, 4096, 512, (4,), ("bf16",), (64, 1024)),
    (307, 700, 128, 64, (2,), ("f32",), (64,)),
]


def families_of(assignment, H):
    if assignment == "mixed":
        return tuple(MIXED[h % len(MIXED)] for h in range(H))
    if assignment == "offsets":
        return tuple("offset+" if h % 2 == 0 else "offset-" for h in range(H))
    if assignment == "flat":
        return ("flat",) * H
    raise ValueError(assignment)


def head_slice(h, H, D):
    hd = D // H
    return slice(h * hd, (h + 1) * hd)


def apply_head_families(c, H, assignment):
    """(q [B, D], kt [B, D, S]) with the assignment's family applied to every head's slice; c is not modified."""
    q = c["q_output"].copy()
    kt = c["kt_cache"].copy()
    D = q.shape[1]
    for h, family in enumerate(families_of(assignment, H)):
        sl = head_slice(h, H, D)
        sub = {"q_output": np.ascontiguousarray(q[:, sl]), "kt_cache": np.ascontiguousarray(kt[:, sl, :]),
               "lengths": c["lengths"]}
        q[:, sl], kt[:, sl, :] = apply_family(sub, family)
    return q, kt


def oracle_heads(oracle, q, kt, v, lengths, H):
    """attention_result [B, D] of the fp32 CPU oracle, head by head on contiguous slices."""
    B, D = q.shape
    out = np.zeros((B, D), np.float32)
    for h in range(H):
        sl = head_slice(h, H, D)
        out[:, sl] = oracle_scan(oracle, np.ascontiguousarray(q[:, sl]), np.ascontiguousarray(kt[:, sl, :]),
                                 np.ascontiguousarray(v[:, :, sl]), lengths)[2]
    return out


class HeadsModel:
    """float64 attention per head and its condition scale per (row, head)."""

    def __init__(self, q, kt, v, lengths, H):
        B, D = q.shape
        self.H, self.D = H, D
        self.lengths = np.asarray(lengths).astype(np.int64)
        self.o = np.zeros((B, D), np.float64)
        self.o_scale = np.zeros((B, H), np.float64)
        for h in range(H):
            sl = head_slice(h, H, D)
            p = fm.softmax(fm.scores(q[:, sl], kt[:, sl, :], lengths), lengths)
            self.o[:, sl] = fm.attend(p, v[:, :, sl], lengths)
            self.o_scale[:, h] = fm.attend_abs(p, v[:, :, sl], lengths).max(axis=1)


def heads_error(o, model):
    """[B, H]: max_d |o - o^| / max_d sum_s p^_s |v_sd| over the head's columns (inf for a non-finite value, and for a
    row of length 0 that is not exactly 0)."""
    o = np.asarray(o)
    B = o.shape[0]
    err = np.zeros((B, model.H), np.float64)
    for h in range(model.H):
        sl = head_slice(h, model.H, model.D)
        for b in range(B):
            g = o[b, sl].astype(np.float64)
            if model.lengths[b] == 0:
                err[b, h] = np.inf if g.any() else 0.0
            elif not np.isfinite(g).all():
                err[b, h] = np.inf
            else:
                err[b, h] = np.abs(g - model.o[b, sl]).max() / model.o_scale[b, h]
    return err


def compare(o, o_oracle, model, assignment, what="", report=print):
    """The comparison of every multi-head test: per score family, the worst (row, head) error of `o` against the
    tolerance derived from the oracle's error on the heads of that family.  Returns [(family, worst, tolerance)]; every
    figure is reported before the caller asserts."""
    err, e_or = heads_error(o, model), heads_error(o_oracle, model)
    fams = families_of(assignment, model.H)
    out = []
    for family in sorted(set(fams)):
        cols = [h for h in range(model.H) if fams[h] == family]
        tol = fm.tolerance(e_or[:, cols])
        worst = float(err[:, cols].max())
        report(f"HEADS {what} | {assignment}/{family}: got {worst:.3e}  oracle {float(e_or[:, cols].max()):.3e}  tol {tol:.3e}")
        out.append((family, worst, tol))
    return out


def assert_within(results, what=""):
    bad = [f"{what} [{family}]: {worst:.3e} > tol {tol:.3e}" for family, worst, tol in results if not worst <= tol]
    assert not bad, "\n".join(bad)


# ---- wrong models: the faults a multi-head kernel actually has ---------------------------------------------------------
def _f64(a):
    return np.asarray(a).astype(np.float64)


def _attend_rows(x, v, lengths):
    return fm.attend(fm.softmax(x, lengths), v, lengths)


def wrong_heads_ignored(q, kt, v, lengths, H):
    """one softmax over the whole embedding width"""
    return _attend_rows(fm.scores(q, kt, lengths), v, lengths)


def wrong_scale_emb_dim(q, kt, v, lengths, H):
    """per head, but divided by sqrt(emb_dim)"""
    D = q.shape[1]
    o = np.zeros(q.shape, np.float64)
    for h in range(H):
        sl = head_slice(h, H, D)
        o[:, sl] = _attend_rows(fm.scores(q[:, sl], kt[:, sl, :], lengths, scale=1.0 / math.sqrt(D)), v[:, :, sl], lengths)
    return o


def wrong_heads_interleaved(q, kt, v, lengths, H):
    """head h owns the columns d % H == h"""
    o = np.zeros(q.shape, np.float64)
    for h in range(H):
        o[:, h::H] = _attend_rows(fm.scores(q[:, h::H], kt[:, h::H, :], lengths), v[:, :, h::H], lengths)
    return o


def wrong_neighbour_probabilities(q, kt, v, lengths, H):
    """head h's probabilities applied to head h + 1's V"""
    D = q.shape[1]
    o = np.zeros(q.shape, np.float64)
    for h in range(H):
        sl, nxt = head_slice(h, H, D), head_slice((h + 1) % H, H, D)
        p = fm.softmax(fm.scores(q[:, sl], kt[:, sl, :], lengths), lengths)
        o[:, nxt] = fm.attend(p, v[:, :, nxt], lengths)
    return o


def wrong_shared_running_max(q, kt, v, lengths, H):
    """a float32 online softmax over pages of 16 whose running maximum is shared by all heads of a row"""
    B, D = q.shape
    hd = D // H
    o = np.zeros((B, D), np.float32)
    with np.errstate(all="ignore"):
        for b in range(B):
            L = int(lengths[b])
            if L == 0:
                continue
            x = np.stack([(q[b, head_slice(h, H, D)].astype(np.float32) @ kt[b, head_slice(h, H, D), :L].astype(np.float32))
                          / np.float32(math.sqrt(hd)) for h in range(H)])               # [H, L]
            m = np.float32(-np.inf)
            l = np.zeros(H, np.float32)
            acc = np.zeros((H, hd), np.float32)
            for s0 in range(0, L, 16):
                xs = x[:, s0:s0 + 16]
                m_new = np.float32(max(m, xs.max()))
                alpha = np.float32(0.0) if m == -np.inf else np.exp(m - m_new)
                p = np.exp(xs - m_new).astype(np.float32)
                l = l * alpha + p.sum(axis=1, dtype=np.float32)
                vs = v[b, s0:min(s0 + 16, L)].astype(np.float32).reshape(-1, H, hd)
                acc = acc * alpha + np.einsum("hs,shd->hd", p, vs).astype(np.float32)
                m = m_new
            o[b] = (acc / l[:, None]).reshape(-1)
    return o


WRONG_MODELS = {"heads ignored": wrong_heads_ignored, "scale 1/sqrt(emb_dim)": wrong_scale_emb_dim,
                "heads interleaved": wrong_heads_interleaved, "neighbour's probabilities": wrong_neighbour_probabilities,
                "shared running maximum": wrong_shared_running_max}


# ---- the CPU engine with heads -------------------------------------------------------------------------------------------
class _HeadsOracle:
    """The oracle module with its attention stages made head-aware: the composition becomes fill + latest + the three
    stages per head, and (for CpuEngine's bf16 mode, which calls the stages itself) the stages run per head.  Everything
    else passes through.  It also records the smallest gap between the two largest logits the decoder has seen."""

    def __init__(self, oracle, n_heads):
        self._o, self._H = oracle, n_heads
        self.min_logit_gap = np.inf
        self._q = self._kt = None

    def __getattr__(self, name):
        return getattr(self._o, name)

    def _attend(self, q, kt, v, lengths, att):
        att[...] = oracle_heads(self._o, q, kt, v, lengths, self._H)

    def self_attention_inference_host(self, inp, lengths, wk, wq, wv, new_idx, kt, v, q, qkt, att, n_new):
        self._o.fill_new_kt_v_cache(inp, new_idx, lengths, wk, wv, kt, v, n_new)
        self._o.get_latest_kt_q_v(inp, lengths, wk, wq, wv, kt, v, q)
        self._attend(q, kt, v, lengths, att)

    def qkt_host(self, q, kt, lengths, qkt):
        self._q, self._kt = q, kt          # the per-head stages run in softmax_v_host, which sees V

    def softmax_in_place_with_lengths_host(self, qkt, lengths):
        pass

    def softmax_v_host(self, qkt, v, att, lengths):
        self._attend(self._q, self._kt, v, lengths, att)

    def decoder_host(self, att, emb_table, score, pos_table, inp, lengths, result):
        live = np.asarray(lengths) > 0
        self._o.decoder_host(att, emb_table, score, pos_table, inp, lengths, result)
        if live.any():
            top2 = np.partition(score[live], -2, axis=1)[:, -2:]
            self.min_logit_gap = min(self.min_logit_gap, float((top2[:, 1] - top2[:, 0]).min()))


class HeadsCpuEngine(CpuEngine):
    """engine_sim.CpuEngine whose attention has n_heads heads; min_logit_gap after a run says how far the greedy token
    choices were from a tie."""

    def __init__(self, oracle, model, items, n_batch, n_sequence, n_heads, bf16=False):
        self.heads_oracle = _HeadsOracle(oracle, n_heads)
        super().__init__(self.heads_oracle, model, items, n_batch, n_sequence, bf16=bf16)

    @property
    def min_logit_gap(self):
        return self.heads_oracle.min_logit_gap


def run_heads_cpu_engine(oracle, model, items, n_batch, n_sequence, n_heads, bf16=False):
    """({item id: all tokens}, smallest top-2 logit gap of the run)."""
    e = HeadsCpuEngine(oracle, model, items, n_batch, n_sequence, n_heads, bf16=bf16)
    while not e.done():
        e.step()
    return e.finished, e.min_logit_gap
