"""The causal multi-query prompt scan and the prompt log-probabilities, for the tests.

The scan.  A segment is (row b, first position p, count n); its query j is position t = p + j of row b and attends slot s of
that row iff s <= t and (no window, or s > t - W, or s < K).  That is the decode problem of a row of length t + 1: query i of a
list becomes VIRTUAL ROW i -- its own q, the K and V of its row, length t + 1 -- and the references are the existing ones on the
virtual rows: gqa_model.model_gqa / oracle_gqa (which are sinks_model's, window_model's and heads_model's on the expanded
operands; with one head and no window the plain float64 model and the plain oracle).  Errors, tolerance and the comparison per
score family are heads_model's: f64_model.tolerance of the fp32 oracle's own error, nothing from a kernel.

The figures.  Entry i of an item's prompt log-probabilities belongs to prompt token i + 1: logprobs_model.reference on the
logits of position i of the float64 forward over the item's tokens (replay_model.Replay with rows 0 .. p - 2), given token
tokens[i + 1].

MUTANTS are the faults such a kernel and its host actually have, each as a wrong model the comparison must reject.

TEST INFRASTRUCTURE, like heads_model.py: never used by the product."""
from types import SimpleNamespace

import numpy as np

import gqa_model as gm
import heads_model as hm
import logprobs_model as lm
import replay_model as rm

# (seed, D, H, Hkv, page type): n_sequence 128 throughout -- the smallest shapes that reach every kernel variant (element type x
# lane loads per row x one head or several): fp32 D 64 (a partly filled lane load), 256, 512 (two lane loads); bf16 D 128, 1024;
# 4 heads at head_dim 32 and 64; 8 heads on 2 and on 1 K/V heads
S = 128
SHAPES = [
    (701, 64, 1, 1, "f32"), (702, 256, 1, 1, "f32"), (703, 512, 1, 1, "f32"), (704, 128, 1, 1, "bf16"), (705, 1024, 1, 1, "bf16"),
    (706, 128, 4, 4, "f32"), (707, 256, 4, 4, "bf16"), (708, 256, 8, 2, "f32"), (709, 512, 8, 1, "bf16"), (710, 1024, 8, 2, "bf16"),
    (711, 512, 4, 4, "f32"),
]
# (window, n_sink): plain, a window of several pages, the same with sinks, a window of a single page
FORMS = ((0, 0), (40, 0), (40, 4), (16, 0))
FAMILIES = ("flat", "peaked", "offset+", "offset-", "late_peak", "early_peak")


def segments_for(tq, n_sequence=S):
    """Segments [(row, first, count)] for a variant of `tq` queries per workgroup, rows in permuted order: counts 1, tq - 1, tq,
    tq + 1 and 2 tq + 1; first positions 0, 15, 16, 17; a query at n_sequence - 1; two segments of one row (a continuation with
    first > 0) -- and the rows each list needs (last scored position + 1 per row)."""
    segs = [(5, 0, 1), (2, 15, tq - 1), (7, 16, tq), (0, 17, tq + 1), (3, 0, 2 * tq + 1), (6, n_sequence - tq - 1, tq + 1),
            (1, 0, tq + 3), (4, 33, 1), (1, tq + 3, 2 * tq), (8, 47, 3 * tq)]
    segs = [s for s in segs if s[2] >= 1]
    n_rows = max(r for r, _, _ in segs) + 1
    lengths = np.zeros(n_rows, np.int32)
    for r, f, n in segs:
        lengths[r] = max(lengths[r], f + n)
    assert lengths.max() == n_sequence and (lengths > 0).all()
    return segs, lengths


def queries(segments):
    """(row, position) of every query, in the dense order of the segments' offsets"""
    rows = np.concatenate([np.full(n, r, np.int64) for r, _, n in segments])
    pos = np.concatenate([np.arange(f, f + n, dtype=np.int64) for _, f, n in segments])
    return rows, pos


def query_vectors(q_rows, rows, pos):
    """One q per query from the row's q: scaled by a factor that differs between the positions of a row, so that two queries
    swapped, or one computed for its neighbour's position, differ beyond any tolerance."""
    return (q_rows[rows] * (1.0 + 0.03125 * (pos % 8))[:, None].astype(np.float32)).astype(np.float32)


def virtual(kt, v, rows, pos):
    """The virtual rows' operands: (kt [n_q, D, S], v [n_q, S, D], lengths t + 1)"""
    return kt[rows], v[rows], (pos + 1).astype(np.int32)


def model_prompt(qv, kt, v, rows, pos, H, Hkv, W, K):
    ktv, vv, Lv = virtual(kt, v, rows, pos)
    return gm.model_gqa(qv, ktv, vv, Lv, H, Hkv, W, K)


def oracle_prompt(oracle, qv, kt, v, rows, pos, H, Hkv, W, K):
    ktv, vv, Lv = virtual(kt, v, rows, pos)
    return gm.oracle_gqa(oracle, qv, ktv, vv, Lv, H, Hkv, W, K)


def scan_float64(qv, kt, v, rows, pos, H, Hkv, W, K):
    """The scan stated directly (a mask per query, a softmax per head): the model the virtual rows are checked against."""
    n, D = qv.shape
    hd, g = D // H, H // Hkv
    out = np.zeros((n, D), np.float64)
    for i in range(n):
        b, t = int(rows[i]), int(pos[i])
        s = np.arange(t + 1)
        m = np.ones(t + 1, bool) if not W else (s > t - W) | (s < K)
        for h in range(H):
            qs, ks = hm.head_slice(h, H, D), hm.head_slice(h // g, H, D)
            x = (qv[i, qs].astype(np.float64) @ kt[b, ks, :t + 1].astype(np.float64)) / np.sqrt(hd)
            x = np.where(m, x, -np.inf)
            p = np.exp(x - x.max())
            out[i, qs] = (p / p.sum()) @ v[b, :t + 1, ks].astype(np.float64)
    return out


# ---- wrong models --------------------------------------------------------------------------------------------------------------
def _with(qv, kt, v, rows, pos, H, Hkv, W, K, lengths=None, lo_shift=0, hi_shift=0, n_sink=None, group=True, positions=None):
    """float64 attention of a scan whose query at position t of a row holding `lengths` tokens attends s <= t + hi_shift (inside
    the row) and (no window, or s > t - W + lo_shift, or s < n_sink), head h on K/V head h // g (group) or h"""
    n, D = qv.shape
    hd, g = D // H, H // Hkv
    pos = pos if positions is None else positions
    out = np.zeros((n, D), np.float64)
    for i in range(n):
        b, t = int(rows[i]), int(pos[i])
        top = t + hi_shift if lengths is None else min(t + hi_shift, int(lengths[b]) - 1)
        s = np.arange(top + 1)
        m = np.ones(top + 1, bool) if not W else (s > t - W + lo_shift) | (s < (K if n_sink is None else n_sink))
        for h in range(H):
            qs, ks = hm.head_slice(h, H, D), hm.head_slice(h // g if group else h, H, D)
            x = np.where(m, (qv[i, qs].astype(np.float64) @ kt[b, ks, :top + 1].astype(np.float64)) / np.sqrt(hd), -np.inf)
            p = np.exp(x - x.max())
            out[i, qs] = (p / p.sum()) @ v[b, :top + 1, ks].astype(np.float64)
    return out


def restarted_positions(segments):
    """positions with the SECOND segment of a row restarted at 0 (a continuation pass that forgets its first position)"""
    seen, out = set(), []
    for r, f, n in segments:
        out.append(np.arange(0, n) if r in seen and f > 0 else np.arange(f, f + n))
        seen.add(r)
    return np.concatenate(out).astype(np.int64)


SCAN_MUTANTS = {
    "the query attends slot t + 1": dict(hi_shift=1),
    "window lower bound one too low": dict(lo_shift=-1),
    "window lower bound one too high": dict(lo_shift=1),
    "sinks dropped": dict(n_sink=0),
    "K/V head h instead of h / g": dict(group=False),
    "second segment restarted at position 0": dict(positions="restarted"),
}


def scan_mutant(name, segments, lengths, qv, kt, v, rows, pos, H, Hkv, W, K):
    """(float64 attention of the wrong scan, whether the fault can show in this form at all)"""
    kw = dict(SCAN_MUTANTS[name])
    applies = True
    if "lo_shift" in kw:
        applies = W > 0
    if "n_sink" in kw:
        applies = W > 0 and K > 0
    if "group" in kw:
        applies = Hkv < H
    if kw.get("positions") == "restarted":
        kw["positions"] = restarted_positions(segments)
        applies = bool((kw["positions"] != pos).any())
    return _with(qv, kt, v, rows, pos, H, Hkv, W, K, lengths=lengths, **kw), applies


# ---- the prompt figures --------------------------------------------------------------------------------------------------------
def prompt_replay(model, tokens, n_prompt, spec):
    """replay_model.Replay over the item's tokens with the logits of the prompt positions 0 .. n_prompt - 2 (position i chooses
    token i + 1)"""
    return rm.Replay(model, np.asarray(tokens, np.int32), spec, rows=np.arange(0, max(int(n_prompt) - 1, 0)))


def given_reference(logits, given, n_top):
    """logprobs_model.reference for tokens the rows are GIVEN: a token outside [0, V) reports -inf for the token and the
    alternatives all the same (logprobs_model.reference reports nothing for a negative token: a head that emitted none)."""
    logits = np.asarray(logits, np.float32)
    given = np.asarray(given, np.int64)
    known = (given >= 0) & (given < logits.shape[1])
    tok_lp, ids, lps = lm.reference(logits, np.where(known, given, 0), n_top)
    return np.where(known, tok_lp, -np.inf), ids, lps


def compare_given(got, logits, given, n_top):
    """logprobs_model.compare against given_reference: (error, tolerance, complaints)"""
    tok_lp, ids, lps = (np.asarray(a) for a in got)
    w_lp, w_ids, w_lps = given_reference(logits, given, n_top)
    bad = []
    err = max(lm.value_error(tok_lp, w_lp), lm.value_error(lps.reshape(w_lps.shape), w_lps) if n_top else 0.0)
    if n_top and not (ids.reshape(w_ids.shape) == w_ids).all():
        bad.append(f"top_ids differ from the model's in rows {np.nonzero((ids.reshape(w_ids.shape) != w_ids).any(axis=1))[0].tolist()}")
        err = np.inf
    if n_top and not bad:
        for b in range(len(w_lp)):
            hit = np.nonzero(w_ids[b] == int(given[b]))[0] if int(given[b]) >= 0 else []
            if len(hit) and np.float32(tok_lp[b]).tobytes() != np.float32(lps.reshape(w_lps.shape)[b, hit[0]]).tobytes():
                bad.append(f"row {b}: the token's logprob is not bit-equal to its entry in the list")
                err = np.inf
    if not np.isfinite(err) and not bad:
        bad.append("a non-finite, padded or out-of-range entry is not as specified")
    return err, lm.tolerance(logits), bad


def prompt_targets(tokens, n_rows, shift=1):
    """the token entry i is scored for: tokens[i + shift] (shift = 1 is right)"""
    return np.asarray([int(tokens[i + shift]) if 0 <= i + shift < len(tokens) else -1 for i in range(n_rows)], np.int64)


def prompt_reference(logits, tokens, n_top, shift=1):
    """(token_logprob [n], top_ids [n, n_top], top_logprobs [n, n_top]) of the prompt positions whose logits these are"""
    return given_reference(logits, prompt_targets(tokens, len(logits), shift), n_top)


def prompt_bound(rep):
    """(2 tol_logit + logprobs_model.tolerance, E32) over the prompt rows, tol_logit as replay_model.judge_item computes it over
    the generated rows: the scaled tolerance of the float32 restatement's error against the float64 forward, plus the rounding
    flips of bf16 / fp8 storage where the spec has them.  Nothing from a kernel."""
    if len(rep.rows) == 0:
        return 0.0, 0.0
    lg = rep.logits
    e32 = float(np.abs(rep.logits32() - lg).max())
    tol_logit = rm._scaled_tolerance(e32, float(np.abs(lg).max()))
    e_flip = rep.flip_envelope(rm.FLIP_ROUNDS, seed=len(rep.x) * 1000003 + len(rep.rows))[1] if rep.spec.flips else 0.0
    return 2.0 * (tol_logit + e_flip) + lm.tolerance(lg.astype(np.float32)), e32


# ---- long prompts: n_sequence 4096 (tests/test_prompt_long_gpu.py, tests/test_prompt_long_cpu.py) -------------------------------
# Dense virtual rows [n_q, D, S] do not fit at S 4096 and D 1024: the rows are a limit_cases.SparseCase and every query is judged
# on its own with limit_cases.row_truth on K[:t + 1], V[:t + 1].
LONG_S = 4096
# (window, n_sink): plain | a dropped run of about 190 pages for the late queries | two sink pages, the second partly live | the
# sink run ends on a page edge | a single-page window | lo <= n_sink for every early query | the hand-off's near side (only the
# query at 4095 drops slot 0) | its far side (the plain mask)
LONG_FORMS = ((0, 0), (1000, 0), (1000, 20), (1000, 16), (16, 0), (24, 40), (4095, 0), (4096, 0))
LONG_MAX_COUNT = 4 * 16 + 3
LONG_K = 150                       # the block at 16 k - 1: its later queries alone see page k
_EDGE_ROWS = (4, 7)


def _edge_window(W):
    """the window whose start the two edge segments are placed by (a window beyond them starts at slot 0 for every query)"""
    return W if 0 < W <= 1000 else 0


def long_segments(tq, W, S=LONG_S):
    """[(row, first, count)] at n_sequence 4096 for a variant of tq queries per workgroup under window W, rows in permuted order:
    the max_count of the call (4 * 16 + 3 queries from position 1000) beside a segment of one query; the last query at
    n_sequence - 1; a continuation starting at 3000; a block on each side of 2047 / 2048; a block at 16 k - 1; a segment whose
    first query's window starts on a page edge (t0 + 1 - W a multiple of 16) and one where it starts at slot 15."""
    e = 1024 + _edge_window(W)
    return [(5, 1000, LONG_MAX_COUNT), (2, 0, 1), (0, S - (3 * tq + 1), 3 * tq + 1), (6, 3000 - (tq + 3), tq + 3),
            (3, 2047 - tq, 2 * tq + 1), (1, 16 * LONG_K - 1, tq + 1), (6, 3000, 2 * tq), (_EDGE_ROWS[0], e - 1, tq + 1),
            (_EDGE_ROWS[1], e + 14, tq + 1)]


def long_reaching_segments(tq):
    """long_segments without the two mid-row blocks and the window-edge segments: the segments that reach the long paths (the
    last query at 4095, the block at 16 k - 1, the max_count segment beside the single query, the continuation at 3000) -- for
    the variants whose truth costs two evaluations per query (the cap, the sink logits); the plain test has the rest"""
    keep = {5, 2, 0, 6, 1}
    return [s for s in long_segments(tq, 0) if s[0] in keep]


def long_lengths(tq, S=LONG_S):
    """tokens per row: the last scored position + 1 over the segment lists of every form (the edge rows' segments move with W)"""
    lengths = np.zeros(8, np.int32)
    for W, _ in LONG_FORMS:
        for r, f, n in long_segments(tq, W, S):
            lengths[r] = max(lengths[r], f + n)
    assert lengths.max() == S and (lengths > 0).all()
    return lengths


def long_families(H, Hkv):
    """{row: families}: one head -- late_peak and early_peak by row (they force the most rescaling: a late peak rescales every
    accumulator at the end of the walk, an early peak is what sinks keep and a window drops); several heads -- the mixed
    assignment of heads_model.ASSIGNMENTS on the K/V heads."""
    if H == 1:
        # row 0 holds the query at n_sequence - 1: with the peak on slots 0 .. 15 the one slot W 4095 drops for it carries weight
        return {0: "early_peak", 1: "late_peak", 3: "late_peak", 4: "early_peak", 5: "late_peak", 6: "early_peak", 7: "late_peak"}
    return {r: hm.families_of("mixed", Hkv) for r in range(8)}


def long_sink_families(Hkv):
    """{row: families} for the scan with sink logits, which takes ONE logit per head for every query of a launch: the families
    whose log-sum-exp stays within a few units from query to query (an offset of 200 or an early peak of 30 times the
    per-position factor of query_vectors moves it by more than that, and the sink would be invisible or total on most
    queries) -- peaked, flat and late_peak (the queries at the end of a row see the peak: every accumulator rescaled at the end
    of the walk; the peak is beyond the band for them, so it is the third K/V head's, where there are four), by K/V head."""
    fams = tuple(("peaked", "flat", "late_peak", "flat")[j % 4] for j in range(Hkv))
    return {r: fams for r in range(8)}


def long_case(seed, D, H, Hkv, tq, families=None):
    import limit_cases as lc
    return lc.SparseCase(seed, long_lengths(tq), LONG_S, D, families=families or long_families(H, Hkv), H=H, Hkv=Hkv, full_rows=True)


def _signature(t, W, K):
    """what the attended set of query t depends on"""
    lo = max(0, t + 1 - W) if W > 0 else 0
    return (t, lo, min(K, lo) if lo > 0 else 0)


def long_truth(oracle, case, values_of, qv, rows, pos, H, Hkv, W, K, cap=None, cache=None, sink=None):
    """[per query: [(columns, model, oracle attention, family) per head]] by limit_cases.row_truth on the row's first t + 1
    tokens.  cache: a dict shared between the forms of one case and one q -- two forms under which a query attends the same
    slots (W 0 and W 4096; W 4095 for every query but the one at 4095) share its truth.  sink: row_truth's learned sink logits."""
    import limit_cases as lc
    zkey = None if sink is None else np.asarray(sink, np.float32).tobytes()
    cache = {} if cache is None else cache
    held = {}
    out = []
    for i in range(len(rows)):
        b, t = int(rows[i]), int(pos[i])
        key = (i, cap, zkey) + _signature(t, W, K)
        if key not in cache:
            if b not in held:
                held[b] = values_of(b)
            Kb, Vb = held[b]
            assert len(Kb) > t, "the row holds the query's position"
            truth = lc.row_truth(oracle, qv[i], Kb[:t + 1], Vb[:t + 1], H, Hkv, W, K, cap=cap, sink=sink)
            cache[key] = [(cols, SimpleNamespace(o=m.o, o_scale=m.o_scale, lengths=m.lengths), o, case.family(b, h if case.H == H else 0))
                          for h, (cols, m, (_, _, o)) in enumerate(truth)]
        out.append(cache[key])
    return out


def long_compare(got, truth, what="", report=print):
    """[(family, worst, tolerance)] of `got` [n_q, D]: per score family the worst condition-scaled error over (query, head)
    against f64_model.tolerance of the oracle's error on the same tokens.  A query without a truth would be skipped: there is
    none (every query attends at least itself), and that is asserted."""
    import f64_model as fm
    err, e_or = {}, {}
    assert len(truth) == len(got) and all(len(heads) > 0 for heads in truth), "no query is skipped"
    for i, heads in enumerate(truth):
        for cols, model, o, family in heads:
            err.setdefault(family, []).append(float(fm.attention_error(np.asarray(got[i][cols])[None], model)[0]))
            e_or.setdefault(family, []).append(float(fm.attention_error(o, model)[0]))
    out = []
    for family in sorted(err):
        tol = fm.tolerance(np.asarray(e_or[family]))
        worst = float(np.max(err[family]))
        report(f"PROMPT LONG {what} | {family}: got {worst:.3e}  oracle {float(np.max(e_or[family])):.3e}  tol {tol:.3e}")
        out.append((family, worst, tol))
    return out


def long_distance(a, b, truth):
    """{family: worst max_d |a - b| over a head's columns in units of the model's condition scale}"""
    out = {}
    for i, heads in enumerate(truth):
        for cols, model, _, family in heads:
            d = float(np.abs(a[i][cols].astype(np.float64) - b[i][cols]).max() / model.o_scale[0])
            out[family] = max(out.get(family, 0.0), d)
    return out


# wrong models that only long rows can show, beside SCAN_MUTANTS
LONG_MUTANTS = {
    "every fourth page from the fifth on is skipped": "stride",       # a wave that loses its stride
    "the sink run is one page short": "sink_page",                    # slots [16 (ps - 1), n_sink) dropped
    "the dropped run is one page too long": "window_page",            # the first window page lost
}


def long_mutant(name, segments, lengths, qv_i, Kb, Vb, i, pos, H, Hkv, W, K):
    """(float64 attention [D] of query i under the wrong scan, whether the fault changes the slots query i attends)"""
    D = len(qv_i)
    hd, g = D // H, H // Hkv
    t = int(pos[i])
    kw = dict(SCAN_MUTANTS.get(name, {}))
    t_as = int(restarted_positions(segments)[i]) if kw.get("positions") == "restarted" else t
    top = min(t_as + kw.get("hi_shift", 0), len(Kb) - 1)
    s = np.arange(top + 1)
    right = np.arange(t + 1)
    if W > 0:
        lo = max(0, t_as + 1 - W)
        right = right[(right >= max(0, t + 1 - W)) | (right < K)]
        live = (s >= lo + kw.get("lo_shift", 0)) | (s < kw.get("n_sink", K))
        kind = LONG_MUTANTS.get(name)
        ps = -(-K // 16)
        if kind == "sink_page" and K > 0:
            live &= ~((s >= 16 * (ps - 1)) & (s < K) & (s < lo))
        if kind == "window_page" and lo // 16 > min(ps, lo // 16):
            live &= ~((s // 16 == lo // 16) & (s >= K))
        s = s[live]
    if LONG_MUTANTS.get(name) == "stride":
        pages = np.unique(s // 16)
        lost = pages[4::4]
        s = s[~np.isin(s // 16, lost)]
    group = kw.get("group", True)
    applies = not np.array_equal(s, right) or (not group and Hkv < H)
    out = np.zeros(D, np.float64)
    if len(s) == 0:
        return out, True
    whole = len(s) == s[-1] + 1
    Ks, Vs = (Kb[:len(s)], Vb[:len(s)]) if whole else (Kb[s], Vb[s])
    for h in range(H):
        qs, ks = hm.head_slice(h, H, D), hm.head_slice(h // g if group else h, H, D)
        x = (Ks[:, ks].astype(np.float64) @ qv_i[qs].astype(np.float64)) / np.sqrt(hd)
        p = np.exp(x - x.max())
        out[qs] = (p / p.sum()) @ Vs[:, ks].astype(np.float64)
    return out, applies


__all__ = ["S", "SHAPES", "FORMS", "FAMILIES", "segments_for", "queries", "query_vectors", "model_prompt", "oracle_prompt",
           "scan_float64", "scan_mutant", "SCAN_MUTANTS", "prompt_replay", "given_reference", "compare_given", "prompt_targets", "prompt_reference", "prompt_bound"]
