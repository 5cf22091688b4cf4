"""Cases at the rim of the launchers' shape space ("the frontier"): what tests/test_shape_limits_gpu.py runs and
tests/test_shape_limits_cpu.py proves sound without a GPU.

SPARSE CASES.  paged_case / base_case hold dense [B, D, S] caches; 16384 short rows beside one row of 65535 tokens do not
fit that.  SparseCase generates q, K and V per row for the row's own length only, applies the score families of
accuracy_cases.apply_family row by row (and head by head, as heads_model.apply_head_families does), and lays the rows into a
page pool by the layout rule of helpers.pool_index -- restated here, and held against oracle.clone_to_pages bit for bit by
the CPU tests.  Pages per row follow the reference's allocation (ceil(min(L + 1, S) / 16)); the page table is n_sequence / 16
wide and every entry beyond a row's pages points at a NaN page; dead slots inside owned pages are NaN after the conversion to
the page type.  For bf16 / fp8 pages the judge reads the rounded values back from the device.

THE JUDGE is the project's: per (row, head) the condition-scaled error against the float64 model (f64_model.Model on the
tokens the row attends), tolerance f64_model.tolerance of the fp32 CPU oracle's error on the same tokens, per score family;
NaN / Inf is an infinite error; rows of length 0 are exactly 0; no sentinel survives.  A window, sinks and grouped heads only
select which slots and which K / V columns a head attends, so one routine serves every lean entry point.

THE FRONTIER TABLE.  LIMITS holds one row per hand-written acceptance rule of the launchers: where the rule stands in the
code (file and the text of the line, which must stand on exactly one line), the last shape on the near side, the first on the
far side, what must happen on each, and the tests that stand on each side -- the function and, where a side is one
parametrisation of it, the case itself.  tests/test_shape_limits_cpu.py checks the rule texts, that every named function
exists and every named case is in the list its test is parametrised by, and that DESIGN.md holds the table's rows."""
import os
from types import SimpleNamespace

import numpy as np

import f64_model as fm
from accuracy_cases import oracle_scan
from helpers import PAGE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 12345.0
ELEM = {"f32": 0, "bf16": 1, "fp8": 2}
ESIZE = {"f32": 4, "bf16": 2, "fp8": 1}
EPL = {"f32": 4, "bf16": 8, "fp8": 16}          # elements per 16-byte lane load
COUNTER_BYTES = 65536                           # the arrival counters and the ticket in front of the workspace body
BAD_ARG = -22


# ---- sparse cases --------------------------------------------------------------------------------------------------------
def _score_direction(qh):
    q64 = qh.astype(np.float64)
    return (q64 / (q64 ** 2).sum() * np.sqrt(len(qh))).astype(np.float32)


def apply_family_row(q, K, family):
    """accuracy_cases.apply_family on one row (or one head's columns of it), in place: q [d], K [L, d]."""
    if family == "flat":
        return
    if family == "peaked":
        q *= np.float32(12.0)
        return
    u = _score_direction(q)
    L = K.shape[0]
    if family in ("offset+", "offset-"):
        K += np.float32(200.0 if family == "offset+" else -200.0) * u[None, :]
    elif family in ("late_peak", "early_peak"):
        lo, hi = (max(L - 17, 0), max(L - 1, 0)) if family == "late_peak" else (0, min(16, L))
        K[lo:hi] += np.float32(30.0) * u[None, :]
    else:
        raise ValueError(family)


class SparseCase:
    """q [B, D]; K, V of row b as [L_b, D] views (rows(b)); pool [pages, 16, 3, D] float32 with x = 0, K and V laid in by the
    layout rule; table [B, S / 16] of page numbers (-1: none).  families: {row: family or one family per head}; every other
    row is flat."""

    def __init__(self, seed, lengths, S, D, families=None, H=1, Hkv=None, full_rows=False):
        """Hkv < H: grouped heads -- a row's families are one per K/V head, applied to K block j and the group's first query
        head as gqa_model.apply_gqa_families does (the group's other heads are FACTORS[i] times the first where the family
        modifies K).  full_rows: a row may hold n_sequence tokens (the prompt scan scores position n_sequence - 1)."""
        assert S % PAGE == 0 and D % H == 0 and H % (Hkv or H) == 0
        self.S, self.D, self.H, self.Hkv = S, D, H, Hkv or H
        self.lengths = np.asarray(lengths, np.int32).copy()
        assert ((self.lengths >= 0) & (self.lengths < S + bool(full_rows))).all(), "rows keep one slot free, as the reference's do"
        L = self.lengths.astype(np.int64)
        self.B = B = len(L)
        rng = np.random.default_rng(seed)
        self.q = (rng.random((B, D), dtype=np.float32) * 2 - 1).astype(np.float32)
        self.start = np.concatenate([[0], np.cumsum(L)])
        T = int(self.start[-1])
        self.K = (rng.random((T, D), dtype=np.float32) * 2 - 1).astype(np.float32)
        self.V = (rng.random((T, D), dtype=np.float32) * 2 - 1).astype(np.float32)
        self.families = {}
        hd = D // H
        g = H // self.Hkv
        for b, fam in (families or {}).items():
            fams = (fam,) * self.Hkv if isinstance(fam, str) else tuple(fam)
            assert len(fams) == self.Hkv and L[b] > 0
            self.families[int(b)] = tuple(fams[h // g] for h in range(H))
            Kb = self.K[self.start[b]:self.start[b + 1]]
            for j, f in enumerate(fams):
                first = self.q[b, j * g * hd:(j * g + 1) * hd]
                apply_family_row(first, Kb[:, j * hd:(j + 1) * hd], f)
                for i in range(1, g):
                    qh = self.q[b, (j * g + i) * hd:(j * g + i + 1) * hd]
                    if f in ("flat", "peaked"):
                        apply_family_row(qh, None, f)
                    else:
                        qh[:] = np.float32(1.0 + 0.125 * (i % 8)) * first
        # pages: the reference's allocation, from a shuffled pool
        self.row_pages = np.where(L > 0, -(-np.minimum(L + 1, S) // PAGE), 0)
        self.page_start = np.concatenate([[0], np.cumsum(self.row_pages)])
        self.n_pages = int(self.page_start[-1])
        order = rng.permutation(max(self.n_pages, 1))
        self.table = np.full((B, S // PAGE), -1, np.int64)
        rows = np.repeat(np.arange(B), self.row_pages)
        self.table[rows, np.arange(self.n_pages) - self.page_start[rows]] = order[:self.n_pages]
        # tokens -> (page, slot)
        tok_row = np.repeat(np.arange(B), L)
        tok_s = np.arange(T) - self.start[tok_row]
        self.tok_page = self.table[tok_row, tok_s // PAGE]
        self.tok_slot = tok_s % PAGE
        self.pool = np.zeros((max(self.n_pages, 1), PAGE, 3, D), np.float32)
        self.pool[self.tok_page, self.tok_slot, 1] = self.K
        self.pool[self.tok_page, self.tok_slot, 2] = self.V
        # dead slots inside owned pages
        dp, ds = [], []
        live = np.nonzero(L > 0)[0]
        for k in range(PAGE + 1):
            s = L[live] + k
            ok = s < self.row_pages[live] * PAGE
            dp.append(self.table[live[ok], s[ok] // PAGE])
            ds.append(s[ok] % PAGE)
        self.dead_page, self.dead_slot = np.concatenate(dp), np.concatenate(ds)

    def rows(self, b):
        return self.K[self.start[b]:self.start[b + 1]], self.V[self.start[b]:self.start[b + 1]]

    def family(self, b, h=0):
        return self.families.get(int(b), ("flat",) * self.H)[h]

    def table_offsets(self):
        """the page table as float offsets into pool.reshape(-1): what oracle.clone_to_pages and helpers.pool_index take"""
        return np.where(self.table >= 0, self.table * (PAGE * 3 * self.D), -1)

    def dense(self):
        """(kt [B, D, S], v [B, S, D]) zero beyond the rows: the dense builders' form (small cases only)."""
        kt = np.zeros((self.B, self.D, self.S), np.float32)
        v = np.zeros((self.B, self.S, self.D), np.float32)
        for b in range(self.B):
            Kb, Vb = self.rows(b)
            kt[b, :, :len(Kb)] = Kb.T
            v[b, :len(Vb)] = Vb
        return kt, v


def sample_rows(B, named, n=64, seed=77):
    """the named rows plus a fixed random sample of n others"""
    named = sorted({int(b) for b in named})
    rest = np.setdiff1d(np.arange(B), named)
    pick = np.random.default_rng(seed).choice(rest, size=min(n, len(rest)), replace=False) if len(rest) else []
    return named + sorted(int(b) for b in pick)


# ---- the truth of a row ---------------------------------------------------------------------------------------------------
def attended(L, window=0, sinks=0):
    """slots row of length L attends: [max(0, L - window), L) and, with sinks, [0, sinks) -- all of [0, L) without a window"""
    s = np.arange(L)
    if window <= 0:
        return s
    lo = max(0, L - window)
    return s[(s >= lo) | (s < sinks)]


def _biased_head(qh, Kh, Vh, idx, L, slope, cap, dtype):
    """(o [1, hd], o_scale) of one head over the attended slots with every operation in `dtype`, as alibi_model / softcap_model
    state it: x = q . K / sqrt(hd); with a cap x = cap tanh(x / cap); with a slope x += slope (s - (L - 1)); softmax; p . V"""
    qh, Kh, Vh = (np.asarray(a).astype(dtype) for a in (qh, Kh, Vh))
    x = ((Kh @ qh).astype(dtype) / dtype(np.sqrt(len(qh)))).astype(dtype)
    if cap is not None:
        x = (dtype(cap) * np.tanh((x / dtype(cap)).astype(dtype)).astype(dtype)).astype(dtype)
    if slope is not None:
        x = (x + dtype(np.float32(slope)) * (idx - (L - 1)).astype(dtype)).astype(dtype)
    e = np.exp(x - x.max())
    p = (e / e.sum(dtype=dtype)).astype(dtype)
    return (p @ Vh).astype(dtype)[None], float((p.astype(np.float64) @ np.abs(Vh.astype(np.float64))).max())


def _sunk_head(qh, Kh, Vh, z, dtype):
    """(o [1, hd], o_scale) of one head over the attended slots with the learned sink logit z (finite or -inf), every
    operation in `dtype`, as attention_sink_logits.hpp and sink_logits_model state it: x = q . K / sqrt(hd); m = max(max x, z);
    o = sum exp(x - m) V / (sum exp(x - m) + exp(z - m)) -- one more logit of the softmax without a value row.  The condition
    scale is 1 where the sink takes the whole mass (the value is then exactly 0), as sink_logits_model's is."""
    qh, Kh, Vh = (np.asarray(a).astype(dtype) for a in (qh, Kh, Vh))
    x = ((Kh @ qh).astype(dtype) / dtype(np.sqrt(len(qh)))).astype(dtype)
    z = dtype(np.float32(z))
    m = np.maximum(x.max(), z)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(x - m)
        ez = np.exp(z - m)
    denom = (e.sum(dtype=dtype) + ez).astype(dtype)
    p = (e / denom).astype(dtype)
    scale = float((p.astype(np.float64) @ np.abs(Vh.astype(np.float64))).max())
    return (p @ Vh).astype(dtype)[None], scale if scale > 0 else 1.0


def row_truth(oracle, q, K, V, H=1, Hkv=None, window=0, sinks=0, slopes=None, cap=None, sink=None):
    """[(columns, f64_model.Model, (x, p, o) of the fp32 oracle)] per head for one row: q [D], K / V [L, D] as the pages hold
    them.  Head h attends the slots attended(L, window, sinks) with K / V head h // (H // Hkv).
    slopes [H] (ALiBi: slopes[h] * (s - (L - 1)) is added to the scaled score of slot s) or cap (soft-capping: the scaled score
    x becomes cap * tanh(x / cap), before the mask): the model is then the float64 evaluation of that expression (o, o_scale
    and lengths, what f64_model.attention_error reads) and the oracle's place is taken by the same expression in float32
    numpy, as alibi_model / softcap_model take their tolerance: (None, None, o32).
    sink [H] float32, each finite or -inf (learned attention-sink logits: _sunk_head): the same arrangement; never beside
    slopes or a cap, as the launchers have it."""
    assert sink is None or (slopes is None and cap is None), "no model defines a sink logit beside a position bias or a cap"
    D = len(q)
    hd = D // H
    g = H // (Hkv or H)
    L = K.shape[0]
    idx = attended(L, window, sinks)
    K, V = (K, V) if len(idx) == L else (K[idx], V[idx])
    out = []
    for h in range(H):
        cols = slice(h * hd, (h + 1) * hd)
        kv = slice((h // g) * hd, (h // g + 1) * hd)
        if sink is not None:
            z = np.asarray(sink, np.float32)[h]
            o64, scale = _sunk_head(q[cols], K[:, kv], V[:, kv], z, np.float64)
            o32, _ = _sunk_head(q[cols], K[:, kv], V[:, kv], z, np.float32)
            model = SimpleNamespace(o=o64, o_scale=np.asarray([scale]), lengths=np.asarray([len(idx)], np.int64))
            out.append((cols, model, (None, None, o32)))
            continue
        if slopes is not None or cap is not None:
            slope = None if slopes is None else np.asarray(slopes, np.float32)[h]
            o64, scale = _biased_head(q[cols], K[:, kv], V[:, kv], idx, L, slope, cap, np.float64)
            o32, _ = _biased_head(q[cols], K[:, kv], V[:, kv], idx, L, slope, cap, np.float32)
            model = SimpleNamespace(o=o64, o_scale=np.asarray([scale]), lengths=np.asarray([len(idx)], np.int64))
            out.append((cols, model, (None, None, o32)))
            continue
        qh = np.ascontiguousarray(q[cols])[None]
        kt = np.ascontiguousarray(K[:, kv].T)[None]
        v = np.ascontiguousarray(V[:, kv])[None]
        n = np.asarray([len(idx)], np.int32)
        out.append((cols, fm.Model(qh, kt, v, n), oracle_scan(oracle, qh, kt, v, n)))
    return out


def largest_score(case, H=1, Hkv=None):
    """softcap_model.largest_score on sparse rows: the largest |q_h . K_{h // g}[s] / sqrt(hd)| over every token of every row"""
    hd, g = case.D // H, H // (Hkv or H)
    tok_row = np.repeat(np.arange(case.B), case.lengths.astype(np.int64))
    top = 0.0
    for h in range(H):
        q = case.q[tok_row, h * hd:(h + 1) * hd].astype(np.float64)
        k = case.K[:, (h // g) * hd:(h // g + 1) * hd].astype(np.float64)
        top = max(top, float(np.abs((q * k).sum(axis=1)).max()) / np.sqrt(hd))
    return top


def scaled_q(case, target, H=1, Hkv=None):
    """softcap_model.scale_q on sparse rows: case.q (float32) scaled so that largest_score is `target`"""
    return (case.q * np.float32(target / largest_score(case, H, Hkv))).astype(np.float32)


def judged_lse(case, values_of, rows, H, Hkv=None, window=0, sinks=0, q=None, lengths=None):
    """[len(rows), H] float64: log sum_{s attended} exp(x_s) of every judged (row, head), -inf for a row of length 0 --
    sink_logits_model.log_sum_exp on sparse rows.  lengths: the tokens of each judged row that count, where that is not the
    row's own length (the prompt scan: a query at position t attends the row's first t + 1 tokens); q: [len(rows), D] then."""
    hd, g = case.D // H, H // (Hkv or H)
    out = np.full((len(rows), H), -np.inf)
    held = {}
    for i, b in enumerate(rows):
        n = int(case.lengths[b] if lengths is None else lengths[i])
        if n == 0:
            continue
        if b not in held:
            held[b] = values_of(b)[0]
        idx = attended(n, window, sinks)
        Kb = held[b][:n][idx].astype(np.float64)
        qb = (case.q[b] if q is None else q[i] if lengths is not None else q[b]).astype(np.float64)
        for h in range(H):
            x = Kb[:, (h // g) * hd:(h // g + 1) * hd] @ qb[h * hd:(h + 1) * hd] / np.sqrt(hd)
            out[i, h] = x.max() + np.log(np.exp(x - x.max()).sum())
    return out


def learned_sparse(lse):
    """sink_logits_model.learned on sparse rows: per head the median of judged_lse over the judged non-empty rows plus that
    module's per-head offset, float32 [H]"""
    from sink_logits_model import head_offsets
    live = np.isfinite(lse[:, 0])
    centre = np.median(lse[live], axis=0) if live.any() else np.zeros(lse.shape[1])
    return (centre + head_offsets(lse.shape[1])).astype(np.float32)


def sink_share(lse, sink):
    """[len(rows), H] float64: the sink's share of every judged (row, head)'s softmax, exp(z - m) / (sum exp(x - m) + exp(z - m))
    = 1 / (1 + exp(lse - z)) -- sink_logits_model.SinkLogitsModel.share on sparse rows; NaN for a row of length 0"""
    z = np.asarray(sink, np.float32).astype(np.float64)[None, :]
    with np.errstate(over="ignore", invalid="ignore"):
        share = 1.0 / (1.0 + np.exp(lse - z))
    return np.where(np.isfinite(lse), share, np.nan)


def biting(lse, sink, what="", heads=None):
    """sink_logits_model.conditioned on sparse rows: asserts that the sink's share lies in SHARE_BAND on at least MIN_BITING of
    the judged non-empty (row, head) pairs of `heads` (default: every head whose logit is finite and below 1e29 in magnitude --
    the -inf, +-1e30 anchors are judged by their own assertions and do not count); returns the fraction"""
    from sink_logits_model import MIN_BITING, SHARE_BAND
    z = np.asarray(sink, np.float32)
    heads = [h for h in range(len(z)) if np.isfinite(z[h]) and abs(z[h]) < 1e29] if heads is None else list(heads)
    s = sink_share(lse, sink)[:, heads]
    s = s[np.isfinite(s)]
    assert s.size, f"{what}: no judged pair carries a finite learned logit"
    f = float(((s >= SHARE_BAND[0]) & (s <= SHARE_BAND[1])).mean())
    assert f >= MIN_BITING, f"{what}: the sink's share lies in {SHARE_BAND} on {f:.2f} of the judged (row, head) pairs only"
    return f


def judge_rows(oracle, case, values_of, got, rows, H=1, Hkv=None, window=0, sinks=0, slopes=None, cap=None, q=None, sink=None,
               heads=None):
    """{family: (kernel errors, oracle errors)} of attention_result `got` [B, D] over the (row, head) pairs of `rows`;
    values_of(b) = (K, V) as the pages hold them.  Rows of length 0: inf unless exactly 0.  slopes / cap / sink: row_truth's;
    q: the queries the launch was given where they are not case.q (scaled_q); heads: the heads judged (default: all)."""
    q = case.q if q is None else q
    out = {}
    for b in rows:
        if case.lengths[b] == 0:
            e = np.inf if np.asarray(got[b]).any() else 0.0
            rec = out.setdefault("flat", ([], []))
            rec[0].append(e)
            rec[1].append(0.0)
            continue
        K, V = values_of(b)
        for h, (cols, model, (_, _, o)) in enumerate(row_truth(oracle, q[b], K, V, H, Hkv, window, sinks, slopes, cap, sink)):
            if heads is not None and h not in heads:
                continue
            rec = out.setdefault(case.family(b, h if case.H == H else 0), ([], []))
            rec[0].append(float(fm.attention_error(np.asarray(got[b][cols])[None], model)[0]))
            rec[1].append(float(fm.attention_error(o, model)[0]))
    return out


# ---- the cases the sink-logit kernels run at the frontier, shared by the GPU tests and their small siblings on the CPU ---------
def heads_case(D, B=16384):
    """(B, 64, D): rows 0, B / 2 - 1 and B - 1 with 63 tokens, lengths 0, 1, 16 .. 18, 20, 21, 33 around the window and sink
    edges, the rest 0 .. 40 tokens with four in ten empty; (case, the named rows)"""
    rng = np.random.default_rng(4600)
    L = rng.integers(0, 41, size=B).astype(np.int32)
    L[rng.random(B) < 0.4] = 0
    named = {0: 63, B // 2 - 1: 63, B - 1: 63, 1: 0, 2: 1, 3: 16, 4: 17, 5: 18, 6: 21, 7: 33, B - 2: 20, B - 3: 0}
    for b, n in named.items():
        L[b] = n
    return SparseCase(4601, L, 64, D), sorted(named)


def merge_case(lengths=(16383, 129)):
    """bf16 (., 16384, 1024) with 32 heads: early_peak on odd heads, late_peak on even ones"""
    fams = tuple("early_peak" if h % 2 else "late_peak" for h in range(32))
    return SparseCase(4700, list(lengths), 16384, 1024, families={b: fams for b in range(len(lengths))}, H=32)


def wide_case(D, flat=False):
    """flat: no score families -- the sink-logit launches take one logit per head for the whole batch, and the condition on it
    (biting) needs rows whose log-sum-exp lie within a few units of each other"""
    fams = None if flat else {6: "late_peak", 7: "offset-", 4: "early_peak"}
    return SparseCase(4200 + D, [0, 1, 16, 17, 63, 64, 127, 100], 128, D, families=fams)


def window_case(D=64, flat=False):
    """flat: as wide_case's"""
    fams = None if flat else {11: "late_peak", 10: "offset-"}
    return SparseCase(4980, [0, 1, 2, 15, 16, 17, 31, 32, 33, 48, 62, 63], 64, D, families=fams)


# the score families against the sink: (., 1024, 256) with 8 heads on 2 K/V heads; a K/V head keeps ONE family over all rows (its
# query heads have one logit each for the whole launch), so the six families are three cases of two
SINK_FAMILY_PAIRS = (("flat", "peaked"), ("offset+", "offset-"), ("late_peak", "early_peak"))


def sink_family_case(pair, B=24):
    """lengths 1, 63, 64, 65, 1008, 1023, 0 and random ones in 1 .. 1023; K/V head j of every row in family pair[j]"""
    i = SINK_FAMILY_PAIRS.index(tuple(pair))
    L = np.concatenate([[1, 63, 64, 65, 1008, 1023, 0], np.random.default_rng(5800 + i).integers(1, 1024, size=B - 7)]).astype(np.int32)
    return SparseCase(5810 + i, L, 1024, 256, families={b: tuple(pair) for b in range(B) if L[b] > 0}, H=8, Hkv=2)


def whole_output_faults(case, got):
    """what every row owes, judged or not: no sentinel, nothing non-finite, exact zeros for rows of length 0"""
    got = np.asarray(got)
    faults = []
    if (got == SENTINEL).any():
        faults.append(f"rows {np.nonzero((got == SENTINEL).any(axis=1))[0][:8].tolist()} keep the sentinel")
    if not np.isfinite(got).all():
        faults.append(f"rows {np.nonzero(~np.isfinite(got).all(axis=1))[0][:8].tolist()} are not finite")
    empty = case.lengths == 0
    if got[empty].any():
        faults.append(f"empty rows {np.nonzero(empty & got.any(axis=1))[0][:8].tolist()} are not zero")
    return faults


# ---- the equal-shares launcher's LDS, restated (attention_stream.hip, launch_stream_decode) ---------------------------------
ST_MIN_PAGES, ST_WAVES, ST_GRANULE = 16, 4, 64


def stream_maxseg(D, elem):
    du = D // EPL[elem]
    nj = -(-du // 64)
    rpi = (4 if du <= 16 else 2 if du <= 32 else 1) if elem == "fp8" else 1
    row_f = nj * (64 // rpi) * EPL[elem]
    return (4 if row_f <= 512 else 2), row_f


def stream_lds_bytes(B, S, D, elem, n_cu, granule=ST_GRANULE):
    """dynamic LDS of the equal-shares kernel: prefix sums | page pointers of a share | q of a group's rows | wave partials |
    wave (m, l) | the group's lengths | misc"""
    G = 2 * n_cu
    maxseg, row_f = stream_maxseg(D, elem)
    p_max = B * (S // PAGE)
    max_pages_wg = max(-(-p_max // G) + 1, 2 * ST_MIN_PAGES + 1, granule)
    a16 = lambda n: (n + 15) & ~15
    return (a16((B + 1) * 4) + a16(max_pages_wg * 8) + maxseg * D * 4 + maxseg * ST_WAVES * row_f * 4 + maxseg * ST_WAVES * 8 +
            maxseg * 4 + (8 + 3 * maxseg + 1) * 4)


def stream_lds_frontier(B, D, elem, n_cu):
    """(S inside the 64 .. 80 KiB branch, first S beyond 80 KiB) over S = 8192, 10240, .. 24576: the largest S the launcher
    still takes and the next one."""
    sizes = list(range(8192, 24576 + 1, 2048))
    inside = [S for S in sizes if 64 * 1024 < stream_lds_bytes(B, S, D, elem, n_cu) <= 80 * 1024]
    beyond = [S for S in sizes if stream_lds_bytes(B, S, D, elem, n_cu) > 80 * 1024]
    assert inside and beyond and max(inside) < min(beyond), (inside, beyond)
    return max(inside), min(beyond)


# ---- the frontier table ---------------------------------------------------------------------------------------------------
CSRC = "min_llm_inference_amd/csrc/"
GPU, CPU = "test_shape_limits_gpu", "test_shape_limits_cpu"


def on(function, listname=None, item=None):
    """a test that stands on one side of a limit: the function in tests/test_shape_limits_gpu.py and, where the side is one
    parametrisation of it, the list that holds the case and the case itself (tests/test_shape_limits_cpu.py checks both)"""
    return (function, listname, item)


def _limit(name, entry, rule, near, far, near_outcome, far_outcome, near_tests, far_tests):
    return SimpleNamespace(name=name, entry=entry, rule=rule, near=near, far=far, near_outcome=near_outcome,
                           far_outcome=far_outcome, near_tests=tuple(near_tests), far_tests=tuple(far_tests))


REFUSED = "MLI_ERR_BAD_ARG, nothing launched"       # the far side is then the REFUSALS entries that name the limit
NO_RULE = "no rule: the offsets are 64-bit"
# rule = (file, text that stands on exactly one line of it); shapes are (B, S, D) with what else matters spelled out
LIMITS = [
    _limit("arrival counters", "mli_decode_scan_paged, lean",
           (CSRC + "attention_fused.hip", "B <= kMaxArrivalRows"),
           "(16384, 128, 64) chunk_tokens 64", "(16385, 128, 64) chunk_tokens 64",
           "scan_chunked, merged in the scan launch, counters zero",
           "scan_chunked + the combine launch, counters zero (no launch counter tells the two merges apart: the result is the evidence)",
           [on("test_chunked_scan_on_the_last_arrival_counter")], [on("test_chunked_scan_beyond_the_arrival_counters")]),
    _limit("row width, fp32 / bf16", "mli_decode_scan_paged, phases 3 / 5 / 7",
           (CSRC + "attention_fused.hip", "if (nj > 8 ||"),
           "f32 (8, 128, 2048), bf16 (8, 128, 4096)", "f32 D 2052, bf16 D 4104", "scan_chunked, D-split", REFUSED,
           [on("test_widest_rows", "WIDE_SHAPES", ("f32", 2048)), on("test_widest_rows", "WIDE_SHAPES", ("bf16", 4096))], []),
    _limit("row width, fp8", "mli_decode_scan_paged, phases 5 / 7",
           (CSRC + "attention_fused.hip", "(!lean || nj > 2)"),
           "fp8 (8, 128, 2048)", "fp8 D 2064", "scan_chunked, two lane loads", REFUSED,
           [on("test_widest_rows", "WIDE_SHAPES", ("fp8", 2048))], []),
    _limit("merge statistics in the launch's LDS, plain scan", "mli_decode_scan_paged, phases 1 / 3 / 5 / 7",
           (CSRC + "attention_fused.hip", "if (!scan_lds_fits(smem)) return 0;"),
           "(1, 519936, 16) chunk_tokens 64: 8124 pairs, 65024 bytes", "(1, 519952, 16) chunk_tokens 64",
           "scan_chunked; the row right", REFUSED,
           [on("test_statistics_fill_the_launch_lds", "LDS_ROWS", ("scan", ()))], []),
    _limit("merge statistics in the launch's LDS, window", "mli_decode_scan_paged_window / _sinks, one head",
           (CSRC + "attention_window.hpp", "if (!scan_lds_fits(smem)) return MLI_ERR_BAD_ARG;"),
           "(1, 519936, 16) W 519935 chunk_tokens 64: 8124 items", "(1, 519952, 16) W 519951 chunk_tokens 64",
           "scan_heads_window; the row right", REFUSED,
           [on("test_statistics_fill_the_launch_lds", "LDS_ROWS", ("window", (1, 519935)))], []),
    _limit("longest rows the tests reach at every page type", "mli_decode_scan_paged, phases 1 / 3 / 7",
           (CSRC + "scan_plan.hpp", "inline size_t plain_merge_stat_bytes(int S)"),
           "(3, 65536, 64) items of 64 and 1024: grids of 1025 and 65 rows", "-",
           "scan_chunked; 1024 statistics pairs staged in LDS", "(the far side is the row above)",
           [on("test_longest_rows_lean"), on("test_longest_rows_materialising")], []),
    _limit("ordered rows, batch floor", "mli_decode_scan_paged, lean",
           (CSRC + "scan_plan.hpp", "B > 512 &&"),
           "(513, 64, 64)", "(512, 64, 64)", "scan_rows_ordered", "scan_rows_grid_order",
           [on("test_row_order_frontier", "ORDER_SHAPES", (513, 64, 0, "scan_rows_ordered"))],
           [on("test_row_order_frontier", "ORDER_SHAPES", (512, 64, 0, "scan_rows_grid_order"))]),
    _limit("ordered rows, kMaxOrderedRows", "mli_decode_scan_paged, lean",
           (CSRC + "scan_plan.hpp", "B <= kMaxOrderedRows &&"),
           "(2048, 64, 64)", "(2049, 64, 64)", "scan_rows_ordered", "scan_rows_grid_order",
           [on("test_row_order_frontier", "ORDER_SHAPES", (2048, 64, 0, "scan_rows_ordered"))],
           [on("test_row_order_frontier", "ORDER_SHAPES", (2049, 64, 0, "scan_rows_grid_order"))]),
    _limit("ordered rows, kMaxOrderedPages", "mli_decode_scan_paged, lean",
           (CSRC + "scan_plan.hpp", "span / kPlanPage <= kMaxOrderedPages;"),
           "(600, 1024, 64) chunk_tokens 1024", "(600, 1040, 64) chunk_tokens 1024", "scan_rows_ordered",
           "scan_chunked with two items per row, neither rows counter",
           [on("test_row_order_frontier", "ORDER_SHAPES", (600, 1024, 1024, "scan_rows_ordered"))],
           [on("test_row_order_frontier", "ORDER_SHAPES", (600, 1040, 1024, None))]),
    _limit("equal shares, kStMaxRows", "mli_decode_scan_paged, phases 7",
           (CSRC + "attention_stream.hip", "|| B > kStMaxRows) return false;"),
           "(2048, 1024, 64)", "(2049, 1024, 64)", "scan_equal_shares", "scan_chunked",
           [on("test_equal_shares_frontier", "SHARES", (2048, 1024, 64, 1 << 21, True))],
           [on("test_equal_shares_frontier", "SHARES", (2049, 1024, 64, 1 << 21, False))]),
    _limit("equal shares, scan_stream_min_tokens", "mli_decode_scan_paged, phases 7",
           (CSRC + "attention_stream.hip", "return (int64_t)B * S >= g_scan_stream_min;"),
           "(2048, 1024, 64): B S = 2^21", "(2047, 1024, 64)", "scan_equal_shares", "scan_chunked",
           [on("test_equal_shares_frontier", "SHARES", (2048, 1024, 64, 1 << 21, True))],
           [on("test_equal_shares_frontier", "SHARES", (2047, 1024, 64, 1 << 21, False))]),
    _limit("equal shares, kStMinSequence", "mli_decode_scan_paged, phases 7",
           (CSRC + "attention_stream.hip", "S < kStMinSequence ||"),
           "(2048, 1024, 64) min_tokens 0", "(2048, 1008, 64) min_tokens 0", "scan_equal_shares", "scan_chunked",
           [on("test_equal_shares_frontier", "SHARES", (2048, 1024, 64, 0, True))],
           [on("test_equal_shares_frontier", "SHARES", (2048, 1008, 64, 0, False))]),
    _limit("equal shares, statistics staged in the q buffer", "mli_decode_scan_paged, phases 7",
           (CSRC + "attention_stream.hip", "(size_t)ml_per_row * sizeof(float2) > (size_t)maxseg * D * sizeof(float) ||"),
           "f32 (256, 8192, 64)", "f32 (256, 8256, 64)", "scan_equal_shares", "scan_chunked",
           [on("test_equal_shares_frontier", "SHARES", (256, 8192, 64, 1 << 21, True))],
           [on("test_equal_shares_frontier", "SHARES", (256, 8256, 64, 1 << 21, False))]),
    _limit("equal shares, 80 KiB of LDS", "mli_decode_scan_paged, phases 7",
           (CSRC + "attention_stream.hip", "|| smem > 80 * 1024) return 0;"),
           "(2048, S_in, 512) f32 / bf16 / fp8 and (2048, S_in, 1024) bf16, S_in from stream_lds_frontier",
           "the same at S_beyond", "scan_equal_shares through hipFuncSetAttribute", "scan_chunked",
           [on("test_equal_shares_lds_frontier", "LDS_SIDES", "inside")], [on("test_equal_shares_lds_frontier", "LDS_SIDES", "beyond")]),
    _limit("equal shares, a row's triples against its slots", "mli_decode_scan_paged, phases 7",
           (CSRC + "attention_stream.hip", "if (stream_triples_bound(S / kPage) > ceil_div_i(S, 64)) return false;"),
           "every n_sequence >= 1024 under every knob setting", "-", "never the reason of a fall-back",
           "unreachable: enumerated over the knobs' ranges in " + CPU + "::test_the_triples_bound_never_refuses",
           [on("test_equal_shares_frontier", "SHARES", (2048, 1024, 64, 0, True))], []),
    _limit("several heads, kPlanMaxRows", "mli_decode_scan_paged_heads / _window / _sinks / _gqa",
           (CSRC + "scan_plan.hpp", "B > kPlanMaxRows || S <= 0 || S % kPlanPage != 0 || D <= 0 || H < 1"),
           "(16384, 64, 128) H 2; (16384, 128, 64) H 2 with two items", "(16385, 64, 128) H 2", "scan_heads_window", REFUSED,
           [on("test_heads_family_on_the_last_row", "HEAD_FORMS", "heads"), on("test_heads_family_on_the_last_row", "HEAD_FORMS", "gqa"),
            on("test_heads_on_the_last_arrival_counter")], []),
    _limit("one head under a window, kPlanMaxRows", "mli_decode_scan_paged_window / _sinks",
           (CSRC + "scan_plan.hpp", "B > kPlanMaxRows || S <= 0 || S % kPlanPage != 0 || D <= 0) return false;"),
           "(16384, 64, 64) W 17", "(16385, 64, 64) W 17", "scan_heads_window", REFUSED,
           [on("test_heads_family_on_the_last_row", "HEAD_FORMS", "window_one_head"),
            on("test_heads_family_on_the_last_row", "HEAD_FORMS", "sinks_one_head")], []),
    _limit("several heads, kMaxMergeStats", "mli_decode_scan_paged_heads / _window",
           (CSRC + "scan_plan.hpp", "plan_ceil_div(S, kMaxItemTokens) * H > kMaxMergeStats"),
           "bf16 (2, 16384, 1024) H 32: 128 items x 32 heads = 4096 pairs", "bf16 (2, 131088, 1024) H 32",
           "scan_heads_window, items of 128", REFUSED,
           [on("test_merge_statistics_fill_their_lds", "MERGE_FORMS", "heads"), on("test_merge_statistics_fill_their_lds", "MERGE_FORMS", "window")], []),
    _limit("several heads, row width", "mli_decode_scan_paged_heads",
           (CSRC + "scan_plan.hpp", "D / epl > 2 * kPlanWave"),
           "f32 (8, 128, 512) H 4, bf16 (8, 128, 1024) H 8", "bf16 D 1056 H 33, f32 D 544 H 17", "scan_heads_window", REFUSED,
           [on("test_heads_widest_rows", "HEADS_WIDE", ("f32", 512, 4)), on("test_heads_widest_rows", "HEADS_WIDE", ("bf16", 1024, 8))], []),
    _limit("contiguous scan, rows", "mli_decode_scan_contiguous",
           (CSRC + "attention_fused_naive.hip", "B > kMaxArrivalRows / 2"),
           "(8192, 512, 16)", "(8193, 512, 16)", "one launch, counters zero", REFUSED,
           [on("test_contiguous_scan_frontier", "CONTIGUOUS_SHAPES", (8192, 512, 16))], []),
    _limit("contiguous scan, chunks per row", "mli_decode_scan_contiguous",
           (CSRC + "attention_fused_naive.hip", "if (nchunk > kNvWaves * kWave * 2) return 0;"),
           "(2, 131072, 16): 512 chunks", "(2, 131076, 16): 513 chunks", "one launch, 512 pairs staged in 4 KiB", REFUSED,
           [on("test_contiguous_scan_frontier", "CONTIGUOUS_SHAPES", (2, 131072, 16))], []),
    _limit("contiguous scan, kNvChunk", "mli_decode_scan_contiguous",
           (CSRC + "attention_fused_naive.hip", "constexpr int kNvChunk = 256;"),
           "(12, 256, 16): one item per row, no workspace body", "(12, 260, 16): two items and the merge",
           "right, counters untouched", "right, counters zero",
           [on("test_contiguous_scan_frontier", "CONTIGUOUS_SHAPES", (12, 256, 16))],
           [on("test_contiguous_scan_frontier", "CONTIGUOUS_SHAPES", (12, 260, 16))]),
    _limit("contiguous scan, LDS by width", "mli_decode_scan_contiguous",
           (CSRC + "attention_fused_naive.hip", "if (smem + 16 > 64 * 1024) return 0;"),
           "(2, 512, 13052): 65520 + 12 bytes", "(2, 512, 13056)", "one launch", REFUSED,
           [on("test_contiguous_scan_frontier", "CONTIGUOUS_SHAPES", (2, 512, 13052))], []),
    _limit("contiguous scan, 16-byte pieces", "mli_decode_scan_contiguous",
           (CSRC + "attention_fused_naive.hip", "if (B <= 0 || D % 4 != 0 || S % 4 != 0 || D <= 0 || S <= 0) return 0;"),
           "emb_dim and n_sequence multiples of 4: every contiguous case", "(12, 256, 18), (12, 258, 16)", "one launch", REFUSED,
           [on("test_contiguous_scan_frontier", "CONTIGUOUS_SHAPES", (12, 260, 16))], []),
    _limit("contiguous scan, alignment", "mli_decode_scan_contiguous",
           (CSRC + "attention_fused_naive.hip", "if (!aligned16_nv(kt) || !aligned16_nv(v) || !aligned16_nv(out)) return 0;"),
           "16-byte aligned caches: every contiguous case", "kt_cache 4 bytes off", "one launch", REFUSED,
           [on("test_contiguous_scan_frontier", "CONTIGUOUS_SHAPES", (12, 256, 16))], []),
    _limit("standalone qkt_paged, q in LDS", "mli_qkt_paged",
           (CSRC + "attention_scan.hip", "if (smem + 64 > 64 * 1024) return MLI_ERR_BAD_ARG;"),
           "f32 (2, 64, 16360)", "f32 (2, 64, 16364)", "scores right", REFUSED,
           [on("test_standalone_qkt_widest_rows", "QKT_SHAPES", ("paged", "f32", 16360))], []),
    _limit("standalone qkt_paged_bf16, q in LDS", "mli_qkt_paged_bf16",
           (CSRC + "attention_scan_bf16.hip", "if (smem + 64 > 64 * 1024) return MLI_ERR_BAD_ARG;"),
           "bf16 (2, 64, 16360)", "bf16 (2, 64, 16368)", "scores right", REFUSED,
           [on("test_standalone_qkt_widest_rows", "QKT_SHAPES", ("paged", "bf16", 16360))], []),
    _limit("standalone qkt, q in LDS", "mli_qkt",
           (CSRC + "attention_scan.hip", "+ (size_t)D * 4 + 64 > 64 * 1024) return MLI_ERR_BAD_ARG;"),
           "(2, 64, 15344)", "(2, 64, 15345)", "scores right", REFUSED,
           [on("test_standalone_qkt_widest_rows", "QKT_SHAPES", ("naive", "f32", 15344))], []),
    _limit("standalone softmax_v, float4 or scalar rows", "mli_softmax_v",
           (CSRC + "attention_scan.hip", "if (D % 4 == 0) return launch_softmax_v_impl<4, false>(p, v_cache"),
           "(24, 512, 64): float4 loads", "(24, 512, 66): scalar loads", "right", "right",
           [on("test_softmax_v_vector_and_scalar_form", "SOFTMAX_V_SHAPES", (24, 512, 64))],
           [on("test_softmax_v_vector_and_scalar_form", "SOFTMAX_V_SHAPES", (24, 512, 66))]),
    _limit("standalone softmax_v, LDS by width", "mli_softmax_v / _paged / _paged_bf16",
           (CSRC + "attention_scan.hip", "const size_t smem = (size_t)ct * 4 + (size_t)(ct / kPage) * 8 + (size_t)kScanWaves * slice_v * VEC * 4;"),
           "every width: rows wider than two lane loads are swept in slices", "-", "at most 12.5 KiB",
           "unreachable: " + CPU + "::test_softmax_v_lds_does_not_grow_with_the_width",
           [on("test_softmax_v_vector_and_scalar_form", "SOFTMAX_V_SHAPES", (24, 512, 66))], []),
    _limit("window hand-off", "mli_decode_scan_paged_window",
           (CSRC + "scan_plan.hpp", "if (window <= 0 || window >= S) return kScanPlain;"),
           "(12, 64, 64) W 63, and W 1", "W 64", "scan_heads_window; W 1 is V's newest row", "the plain scan: scan_chunked",
           [on("test_window_extremes", "WINDOW_CALLS", ("window", 63, 0, True)), on("test_window_extremes", "WINDOW_CALLS", ("window", 1, 0, True))],
           [on("test_window_extremes", "WINDOW_CALLS", ("window", 64, 0, False))]),
    _limit("sinks hand-off", "mli_decode_scan_paged_sinks",
           (CSRC + "scan_plan.hpp", "return (long long)n_sink + window >= S ? kScanPlain : kScanSinks;"),
           "(12, 64, 64) K 4 W 59", "K 4 W 60", "scan_heads_window", "the plain scan: scan_chunked",
           [on("test_window_extremes", "WINDOW_CALLS", ("sinks", 59, 4, True))], [on("test_window_extremes", "WINDOW_CALLS", ("sinks", 60, 4, False))]),
    _limit("offsets beyond 2^31, three-stage launchers", "mli_qkt_paged, mli_softmax_in_place_with_lengths, mli_softmax_v_paged",
           (CSRC + "attention_scan.hip", ": reinterpret_cast<V*>(dst + ((int64_t)b * nchunk_max + c) * D);"),
           "f32 (16384, 4096, 2048) chunk_tokens 64: partial sums of 8 GiB, rows 16380 .. 16383 live", "-",
           "probabilities and attention of the last rows right", NO_RULE, [on("test_offsets_beyond_2_31_three_stage")], []),
    _limit("offsets beyond 2^31, sampled head", "mli_sample_tokens, mli_sample_tokens_logprobs",
           (CSRC + "decoder_sample.hip", "const int tok = sample_row<LOGPROBS>(logits + (int64_t)b * V,"),
           "[16384, 131072] logits, rows 16376 .. 16383 live", "-", "tokens the reference's, logprobs the model's", NO_RULE,
           [on("test_offsets_beyond_2_31_sampled_head")], []),
    _limit("offsets beyond 2^31, contiguous caches", "mli_decode_scan_contiguous",
           (CSRC + "attention_fused_naive.hip", "const float* base = kt + (int64_t)b * D * S + s;"),
           "(2049, 4096, 256): 2^31 + 2^20 elements per cache, rows 2045 .. 2048 live", "-", "the last rows right", NO_RULE,
           [on("test_offsets_beyond_2_31_contiguous")], []),
    _limit("offsets beyond 2^31, paged partial rows", "mli_decode_scan_paged, phases 7 and 3",
           (CSRC + "scan_item_body.hpp", "float* o = direct ? out + (int64_t)b * D : partial + ((int64_t)b * nchunk_max + c) * D;"),
           "f32 (16384, 4096, 2048) chunk_tokens 64: partial rows of 8 GiB, rows 16380 .. 16383 live", "-",
           "scan_chunked; the last rows right", NO_RULE, [on("test_offsets_beyond_2_31_paged")], []),
    _limit("offsets beyond 2^31, prompt logits", "mli_paged_prompt_logprobs",
           (CSRC + "compose.hip", "p.targets = p.logits + up((size_t)n * V * sizeof(float));"),
           "n_positions 16384, n_vocab 131072, emb_dim 64: logits of 8 GiB inside the scratch, the last eight positions judged", "-",
           "scan_prompt; the figures right", NO_RULE, [on("test_offsets_beyond_2_31_prompt_logits")], []),
    # ---- the prompt scan, ALiBi, rotary embeddings and soft-capping ----
    _limit("prompt scan, one head, row width", "mli_prompt_scan_paged, mli_paged_prompt_logprobs",
           (CSRC + "scan_plan.hpp", "return plan_ceil_div(D / epl, kPlanWave) <= 2;"),
           "f32 (4, 128, 512), bf16 (4, 128, 1024)", "f32 D 516, bf16 D 1032", "scan_prompt, two lane loads", REFUSED,
           [on("test_prompt_scan_widest_rows", "PROMPT_WIDE", ("f32", 512)), on("test_prompt_scan_widest_rows", "PROMPT_WIDE", ("bf16", 1024))], []),
    _limit("prompt scan, rows", "mli_prompt_scan_paged / _softcap",
           (CSRC + "scan_plan.hpp", "if (!window_plain_shape_ok(B, S, D, elem)) return false;"),
           "(16384, 64, 64) H 1 and (16384, 64, 128) H 2, segments on rows 0, 8191 and 16383", "(16385, 64, .)",
           "scan_prompt / scan_prompt_softcap", REFUSED,
           [on("test_prompt_scan_on_the_last_row", "PROMPT_ROWS", (1, None)), on("test_prompt_scan_on_the_last_row", "PROMPT_ROWS", (2, None)),
            on("test_prompt_scan_on_the_last_row", "PROMPT_ROWS", (2, 5.0))], []),
    _limit("prompt scan, page types", "mli_prompt_scan_paged / _softcap, mli_paged_prompt_logprobs",
           (CSRC + "scan_plan.hpp", "if (elem != MLI_ELEM_F32 && elem != MLI_ELEM_BF16) return false;"),
           "fp32 and bf16 pages", "fp8 pages", "scan_prompt", REFUSED,
           [on("test_prompt_scan_widest_rows", "PROMPT_WIDE", ("f32", 512)), on("test_prompt_scan_widest_rows", "PROMPT_WIDE", ("bf16", 1024))], []),
    _limit("prompt scan, window hand-off", "mli_prompt_scan_paged",
           (CSRC + "attention_prompt.hip", "const ScanKind kind = lean_scan_kind(S, window, n_sink);"),
           "(4, 64, 64) W 63; W 4095 at n_sequence 4096 in tests/test_prompt_long_gpu.py", "W 64 (there: W 4096)",
           "scan_prompt; the query at 63 drops slot 0", "scan_prompt with the plain mask: the bits of W 0",
           [on("test_prompt_window_hand_off", "PROMPT_WINDOWS", (63, True))], [on("test_prompt_window_hand_off", "PROMPT_WINDOWS", (64, False))]),
    _limit("prompt scan, grid", "mli_prompt_scan_paged / _softcap, mli_paged_prompt_logprobs",
           (CSRC + "scan_plan.hpp", "return (long long)n_seg * plan_ceil_div(max_count, tq) * (kPlanWaves * kPlanWave) < (1LL << 32);"),
           "2^24 - 1 workgroups (the runtime launches fewer than 2^32 work items per grid dimension); not run at the limit: every prompt case lies inside it",
           "n_seg 32768, max_count 4096 at 8 queries per workgroup: 2^24 workgroups", "scan_prompt", REFUSED,
           [on("test_prompt_scan_on_the_last_row", "PROMPT_ROWS", (1, None))], []),
    _limit("prompt q projection, segments", "mli_prompt_project_q, mli_paged_prompt_logprobs",
           (CSRC + "proj_gemm.hip", "if (max_count < 1 || max_count > S || n_q < 1 || n_seg > 65535) return MLI_ERR_BAD_ARG;"),
           "65535 segments of one position over (16, 4096, 64)", "65536 segments", "gemm_f32_rows64 / gemm_bf16_widened; q right", REFUSED,
           [on("test_prompt_project_q_at_the_last_segment", "PROJECT_ELEMS", "f32"), on("test_prompt_project_q_at_the_last_segment", "PROJECT_ELEMS", "bf16")], []),
    _limit("ALiBi, heads and slopes", "mli_decode_scan_paged_alibi, mli_paged_attention_lean_alibi",
           (CSRC + "compose.hip", "if (n_heads < 2 || slopes == nullptr) return MLI_ERR_BAD_ARG;"),
           "(16384, 64, 128) H 2, H 2 on 1", "H 1; a null slopes pointer", "scan_heads_alibi", REFUSED,
           [on("test_heads_family_on_the_last_row", "HEAD_FORMS", "alibi"), on("test_heads_family_on_the_last_row", "HEAD_FORMS", "alibi_gqa")], []),
    _limit("soft-cap, heads and cap", "mli_decode_scan_paged_softcap, mli_prompt_scan_paged_softcap",
           (CSRC + "compose.hip", "if (n_heads < 2 || !(cap > 0.f) || !std::isfinite(cap)) return MLI_ERR_BAD_ARG;"),
           "(16384, 64, 128) H 2, H 2 on 1, cap 5", "H 1; cap 0, -1, inf, NaN", "scan_heads_softcap", REFUSED,
           [on("test_heads_family_on_the_last_row", "HEAD_FORMS", "softcap"), on("test_heads_family_on_the_last_row", "HEAD_FORMS", "softcap_gqa")], []),
    _limit("sink logits, heads and logits", "mli_decode_scan_paged_sink_logits, mli_paged_attention_lean_sink_logits",
           (CSRC + "compose.hip", "if (n_heads < 2 || sink_logits == nullptr) return MLI_ERR_BAD_ARG;"),
           "(16384, 64, 128) H 2, H 2 on 1, W 17, W 16 K 4", "H 1; a null logits pointer", "scan_heads_sink_logits", REFUSED,
           [on("test_heads_family_on_the_last_row", "HEAD_FORMS", "sink_logits"), on("test_heads_family_on_the_last_row", "HEAD_FORMS", "sink_logits_gqa"),
            on("test_heads_family_on_the_last_row", "HEAD_FORMS", "sink_logits_window"),
            on("test_heads_family_on_the_last_row", "HEAD_FORMS", "sink_logits_sinks")], []),
    _limit("sink logits, heads and logits, prompt scan", "mli_prompt_scan_paged_sink_logits",
           (CSRC + "attention_prompt.hip", "if (sunk && (H < 2 || sink_logits == nullptr)) return MLI_ERR_BAD_ARG;"),
           "(16384, 64, 128) H 2, segments on rows 0, 8191 and 16383; bf16 D 1024 H 8 on 2, f32 D 512 H 4", "H 1; a null logits pointer",
           "scan_prompt_sink_logits", REFUSED,
           [on("test_prompt_scan_on_the_last_row", "PROMPT_ROWS", (2, "sink_logits")),
            on("test_prompt_scan_widest_rows", "PROMPT_WIDE", ("f32", 512)), on("test_prompt_scan_widest_rows", "PROMPT_WIDE", ("bf16", 1024))], []),
    _limit("sink logits, heads and logits, prompt scoring", "mli_paged_prompt_logprobs_sink_logits",
           (CSRC + "compose.hip", "if (sunk && (n_heads < 2 || sink_logits == nullptr)) return MLI_ERR_BAD_ARG;"),
           "the scan behind the scoring at (16384, 64, 128) H 2, segments on rows 0, 8191 and 16383 (the scoring itself: tests/test_sink_logits_prompt_gpu.py)",
           "H 1; a null logits pointer", "scan_prompt_sink_logits", REFUSED,
           [on("test_prompt_scan_on_the_last_row", "PROMPT_ROWS", (2, "sink_logits"))], []),
    _limit("rotary head size", "every *_rope entry point",
           (CSRC + "proj_gemm.hip", "if (table == nullptr || n_heads < 1 || D < 1 || D % n_heads != 0 || (D / n_heads) % 2 != 0) return -1;"),
           "head size 2: (70, 64, 64) H 32", "head size 17 (D 68, H 4) and 33 (D 132, H 4)",
           "gemm_f32_rope / gemm_bf16_rope", REFUSED, [on("test_rope_at_the_smallest_head_size")], []),
]

# Every call the launchers must refuse before anything is launched: (entry point, arguments after the pointers, limit,
# chunk_tokens).  Run with null pointers on the CPU (a launch would fail there, a refusal returns MLI_ERR_BAD_ARG) and with
# launch counters on the GPU.  Entry points: scan(B, S, D, elem, phases) | heads(B, S, D, H, elem) | window(B, S, D, H, W, elem)
# | sinks(B, S, D, H, W, K, elem) | gqa(B, S, D, H, Hkv, W, K, elem) | contiguous(B, S, D), contiguous_kt4: the same with
# kt_cache 4 bytes off | qkt_paged / qkt_paged_bf16 / qkt (B, S, D)
_W, _H, _P = "row width, fp32 / bf16", "several heads, kPlanMaxRows", "merge statistics in the launch's LDS, plain scan"
_PW, _PR, _PT, _PG = "prompt scan, one head, row width", "prompt scan, rows", "prompt scan, page types", "prompt scan, grid"
_AH, _SH, _RH = "ALiBi, heads and slopes", "soft-cap, heads and cap", "rotary head size"
_ZH, _ZS, _ZP = ("sink logits, heads and logits" + s for s in ("", ", prompt scan", ", prompt scoring"))
REFUSALS = [
    ("scan", (8, 128, 2052, 0, 3), _W, 0), ("scan", (8, 128, 2052, 0, 5), _W, 0), ("scan", (8, 128, 2052, 0, 7), _W, 0),
    ("scan", (8, 128, 4104, 1, 3), _W, 0), ("scan", (8, 128, 4104, 1, 5), _W, 0), ("scan", (8, 128, 4104, 1, 7), _W, 0),
    ("scan", (8, 128, 2064, 2, 5), "row width, fp8", 0), ("scan", (8, 128, 2064, 2, 7), "row width, fp8", 0),
    ("scan", (1, 519952, 16, 0, 7), _P, 64), ("scan", (1, 519952, 16, 0, 3), _P, 64), ("scan", (1, 519952, 16, 1, 5), _P, 64),
    ("scan", (1, 519952, 16, 2, 7), _P, 64),
    ("window", (1, 519952, 16, 1, 519951, 0), "merge statistics in the launch's LDS, window", 64),
    ("sinks", (1, 519952, 16, 1, 519940, 4, 1), "merge statistics in the launch's LDS, window", 64),
    ("heads", (16385, 64, 128, 2, 0), _H, 0), ("heads", (16385, 64, 128, 2, 1), _H, 0),
    ("window", (16385, 64, 128, 2, 17, 0), _H, 0), ("sinks", (16385, 64, 128, 2, 16, 4, 0), _H, 0),
    ("gqa", (16385, 64, 128, 2, 1, 0, 0, 0), _H, 0),
    ("window", (16385, 64, 64, 1, 17, 0), "one head under a window, kPlanMaxRows", 0),
    ("sinks", (16385, 64, 64, 1, 16, 4, 2), "one head under a window, kPlanMaxRows", 0),
    ("heads", (2, 131088, 1024, 32, 1), "several heads, kMaxMergeStats", 0),
    ("window", (2, 131088, 1024, 32, 8192, 1), "several heads, kMaxMergeStats", 0),
    ("heads", (2, 64, 1056, 33, 1), "several heads, row width", 0), ("heads", (2, 64, 544, 17, 0), "several heads, row width", 0),
    ("contiguous", (8193, 512, 16), "contiguous scan, rows", 0),
    ("contiguous", (2, 131076, 16), "contiguous scan, chunks per row", 0),
    ("contiguous", (2, 512, 13056), "contiguous scan, LDS by width", 0),
    ("contiguous", (12, 256, 18), "contiguous scan, 16-byte pieces", 0), ("contiguous", (12, 258, 16), "contiguous scan, 16-byte pieces", 0),
    ("contiguous_kt4", (12, 256, 16), "contiguous scan, alignment", 0),
    ("qkt_paged", (2, 64, 16364), "standalone qkt_paged, q in LDS", 0),
    ("qkt_paged_bf16", (2, 64, 16368), "standalone qkt_paged_bf16, q in LDS", 0),
    ("qkt", (2, 64, 15345), "standalone qkt, q in LDS", 0),
    # the prompt scan: prompt / prompt_softcap (n_seg, max_count, n_q, B, S, D, H, Hkv, W, K[, cap], elem) |
    # prompt_logprobs (n_seg, max_count, n_positions, B, S, D, V, H, Hkv, W, K, elem) | prompt_project_q (n_seg, max_count, n_q, B, S, D, elem)
    ("prompt", (1, 1, 1, 4, 128, 516, 1, 1, 0, 0, 0), _PW, 0), ("prompt", (1, 1, 1, 4, 128, 1032, 1, 1, 0, 0, 1), _PW, 0),
    ("prompt_logprobs", (1, 1, 1, 4, 128, 516, 1030, 1, 1, 0, 0, 0), _PW, 0), ("prompt_logprobs", (1, 1, 1, 4, 128, 1032, 1030, 1, 1, 40, 4, 1), _PW, 0),
    ("prompt", (1, 1, 1, 16385, 64, 64, 1, 1, 0, 0, 0), _PR, 0), ("prompt", (1, 1, 1, 16385, 64, 64, 1, 1, 17, 0, 1), _PR, 0),
    ("prompt", (1, 1, 1, 16385, 64, 128, 2, 2, 0, 0, 0), _PR, 0), ("prompt", (1, 1, 1, 16385, 64, 128, 2, 1, 0, 0, 1), _PR, 0),
    ("prompt_softcap", (1, 1, 1, 16385, 64, 128, 2, 2, 0, 0, 5.0, 0), _PR, 0),
    ("prompt_logprobs", (1, 1, 1, 16385, 64, 64, 512, 1, 1, 0, 0, 0), _PR, 0),
    ("prompt", (1, 1, 1, 4, 128, 64, 1, 1, 0, 0, 2), _PT, 0), ("prompt", (1, 1, 1, 4, 128, 128, 2, 2, 0, 0, 2), _PT, 0),
    ("prompt_softcap", (1, 1, 1, 4, 128, 128, 2, 2, 0, 0, 5.0, 2), _PT, 0), ("prompt_logprobs", (1, 1, 1, 4, 128, 64, 512, 1, 1, 0, 0, 2), _PT, 0),
    ("prompt", (32768, 4096, 1, 8, 4096, 64, 1, 1, 0, 0, 0), _PG, 0), ("prompt", (32768, 4096, 1, 8, 4096, 128, 4, 4, 1000, 20, 0), _PG, 0),
    ("prompt", (16384, 4096, 1, 8, 4096, 1024, 1, 1, 0, 0, 1), _PG, 0), ("prompt_softcap", (8192, 4096, 1, 8, 4096, 1024, 16, 2, 0, 0, 5.0, 1), _PG, 0),
    ("prompt_logprobs", (32768, 4096, 1, 8, 4096, 64, 512, 1, 1, 0, 0, 0), _PG, 0),
    ("prompt_logprobs", (16384, 4096, 1, 8, 4096, 1024, 512, 1, 1, 0, 0, 1), _PG, 0),
    ("prompt_logprobs", (65536, 1, 65536, 16, 4096, 64, 512, 1, 1, 0, 0, 0), "prompt q projection, segments", 0),
    ("prompt_project_q", (65536, 1, 65536, 16, 4096, 64, 0), "prompt q projection, segments", 0),
    ("prompt_project_q", (65536, 1, 65536, 16, 4096, 64, 1), "prompt q projection, segments", 0),
    # alibi (B, S, D, H, Hkv, W, K, slopes given?, elem) | softcap (B, S, D, H, Hkv, W, K, cap, elem)
    ("alibi", (8, 64, 128, 1, 1, 0, 0, True, 0), _AH, 0), ("alibi", (8, 64, 64, 1, 1, 17, 0, True, 1), _AH, 0),
    ("alibi", (8, 64, 128, 2, 2, 0, 0, False, 0), _AH, 0), ("alibi", (8, 64, 128, 2, 1, 16, 4, False, 1), _AH, 0),
    ("softcap", (8, 64, 128, 1, 1, 0, 0, 5.0, 0), _SH, 0), ("softcap", (8, 64, 128, 2, 2, 0, 0, 0.0, 0), _SH, 0),
    ("softcap", (8, 64, 128, 2, 2, 0, 0, -1.0, 1), _SH, 0), ("softcap", (8, 64, 128, 2, 1, 17, 0, float("inf"), 0), _SH, 0),
    ("softcap", (8, 64, 128, 2, 2, 16, 4, float("nan"), 0), _SH, 0),
    ("prompt_softcap", (1, 1, 1, 4, 128, 128, 1, 1, 0, 0, 5.0, 0), _SH, 0), ("prompt_softcap", (1, 1, 1, 4, 128, 128, 2, 2, 0, 0, 0.0, 0), _SH, 0),
    ("prompt_softcap", (1, 1, 1, 4, 128, 128, 2, 2, 0, 0, float("nan"), 1), _SH, 0),
    # latest_rope (B, S, D, H, elem) | fill_rope (B, S, D, n_new, H, elem) | prefill_rope (B, S, D, n_new, W, K, H, elem) |
    # lean_rope (B, S, D, n_new, H, Hkv, W, K, elem): a table pointer that is not null, head sizes 17 and 33
    ("latest_rope", (8, 64, 68, 4, 0), _RH, 0), ("latest_rope", (8, 64, 132, 4, 0), _RH, 0), ("latest_rope", (8, 64, 136, 8, 1), _RH, 0),
    ("latest_rope", (8, 64, 272, 16, 2), _RH, 0),
    ("fill_rope", (8, 64, 68, 2, 4, 0), _RH, 0), ("fill_rope", (8, 64, 136, 2, 8, 1), _RH, 0), ("fill_rope", (8, 64, 132, 2, 4, 0), _RH, 0),
    ("prefill_rope", (8, 64, 68, 2, 0, 0, 4, 0), _RH, 0), ("prefill_rope", (8, 64, 136, 2, 32, 4, 8, 1), _RH, 0),
    ("prefill_rope", (8, 64, 272, 2, 0, 0, 16, 2), _RH, 0),
    ("lean_rope", (8, 64, 68, 2, 4, 4, 0, 0, 0), _RH, 0), ("lean_rope", (8, 64, 132, 2, 4, 2, 17, 0, 0), _RH, 0),
    # sink_logits / lean_sink_logits (B, S, D, H, Hkv, W, K, logits given?, elem) | prompt_sink_logits (n_seg, max_count, n_q, B, S,
    # D, H, Hkv, W, K, logits given?, elem) | prompt_logprobs_sink_logits (n_seg, max_count, n_positions, B, S, D, V, H, Hkv, W, K,
    # logits given?, elem).  One head and null logits are the rule's own far side; fp8 pages, head size 48 and K/V heads that do
    # not divide the heads are what the front refuses right behind it (no sink logit exists there); the rest are the shared
    # plans' limits, reached through the sink-logit entry points.
    ("sink_logits", (8, 64, 128, 1, 1, 0, 0, True, 0), _ZH, 0), ("sink_logits", (8, 64, 64, 1, 1, 17, 0, True, 1), _ZH, 0),
    ("sink_logits", (8, 64, 128, 2, 2, 0, 0, False, 0), _ZH, 0), ("sink_logits", (8, 64, 128, 2, 1, 16, 4, False, 1), _ZH, 0),
    ("sink_logits", (8, 64, 128, 2, 2, 0, 0, True, 2), _ZH, 0), ("sink_logits", (8, 64, 96, 2, 2, 0, 0, True, 0), _ZH, 0),
    ("sink_logits", (8, 64, 256, 8, 3, 0, 0, True, 1), _ZH, 0),
    ("sink_logits", (16385, 64, 128, 2, 2, 0, 0, True, 0), _H, 0), ("sink_logits", (16385, 64, 128, 2, 1, 17, 0, True, 1), _H, 0),
    ("sink_logits", (2, 64, 1056, 33, 33, 0, 0, True, 1), "several heads, row width", 0),
    ("sink_logits", (2, 131088, 1024, 32, 32, 0, 0, True, 1), "several heads, kMaxMergeStats", 0),
    ("sink_logits", (2, 131088, 1024, 32, 8, 8192, 0, True, 1), "several heads, kMaxMergeStats", 0),
    ("lean_sink_logits", (8, 64, 128, 1, 1, 0, 0, True, 0), _ZH, 0), ("lean_sink_logits", (8, 64, 128, 2, 2, 0, 0, False, 0), _ZH, 0),
    ("lean_sink_logits", (8, 64, 128, 2, 2, 16, 4, True, 2), _ZH, 0), ("lean_sink_logits", (8, 64, 96, 2, 2, 0, 0, True, 1), _ZH, 0),
    ("lean_sink_logits", (8, 64, 256, 8, 3, 0, 0, True, 0), _ZH, 0),
    ("lean_sink_logits", (16385, 64, 128, 2, 2, 0, 0, True, 0), _H, 0),
    ("lean_sink_logits", (2, 64, 1056, 33, 33, 0, 0, True, 1), "several heads, row width", 0),
    ("lean_sink_logits", (2, 131088, 1024, 32, 32, 0, 0, True, 1), "several heads, kMaxMergeStats", 0),
    ("prompt_sink_logits", (1, 1, 1, 4, 128, 128, 1, 1, 0, 0, True, 0), _ZS, 0), ("prompt_sink_logits", (1, 1, 1, 4, 128, 128, 2, 2, 0, 0, False, 0), _ZS, 0),
    ("prompt_sink_logits", (1, 1, 1, 4, 128, 128, 2, 1, 40, 4, False, 1), _ZS, 0),
    ("prompt_sink_logits", (1, 1, 1, 4, 128, 128, 2, 2, 0, 0, True, 2), _PT, 0), ("prompt_sink_logits", (1, 1, 1, 4, 128, 96, 2, 2, 0, 0, True, 0), _ZS, 0),
    ("prompt_sink_logits", (1, 1, 1, 4, 128, 256, 8, 3, 0, 0, True, 1), _ZS, 0),
    ("prompt_sink_logits", (1, 1, 1, 16385, 64, 128, 2, 2, 0, 0, True, 0), _PR, 0), ("prompt_sink_logits", (1, 1, 1, 16385, 64, 128, 2, 1, 17, 0, True, 1), _PR, 0),
    ("prompt_sink_logits", (1, 1, 1, 2, 64, 1056, 33, 33, 0, 0, True, 1), "several heads, row width", 0),
    ("prompt_sink_logits", (1, 1, 1, 2, 131088, 1024, 32, 32, 0, 0, True, 1), "several heads, kMaxMergeStats", 0),
    ("prompt_sink_logits", (32768, 4096, 1, 8, 4096, 128, 4, 4, 1000, 20, True, 0), _PG, 0),
    ("prompt_sink_logits", (8192, 4096, 1, 8, 4096, 1024, 16, 2, 0, 0, True, 1), _PG, 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 4, 128, 128, 512, 1, 1, 0, 0, True, 0), _ZP, 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 4, 128, 128, 512, 2, 2, 0, 0, False, 0), _ZP, 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 4, 128, 128, 512, 2, 1, 40, 4, False, 1), _ZP, 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 4, 128, 128, 512, 2, 2, 0, 0, True, 2), _PT, 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 4, 128, 96, 512, 2, 2, 0, 0, True, 0), _ZP, 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 4, 128, 256, 512, 8, 3, 0, 0, True, 1), _ZP, 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 16385, 64, 128, 512, 2, 2, 0, 0, True, 0), _PR, 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 2, 64, 1056, 512, 33, 33, 0, 0, True, 1), "several heads, row width", 0),
    ("prompt_logprobs_sink_logits", (1, 1, 1, 2, 131088, 1024, 512, 32, 32, 0, 0, True, 1), "several heads, kMaxMergeStats", 0),
    ("prompt_logprobs_sink_logits", (32768, 4096, 1, 8, 4096, 128, 512, 4, 4, 0, 0, True, 0), _PG, 0),
    ("prompt_logprobs_sink_logits", (8192, 4096, 1, 8, 4096, 1024, 512, 16, 2, 0, 0, True, 1), _PG, 0),
]


def call_refusal(lib, entry, args, workspace=None, workspace_bytes=1 << 40, stream=None, data=None):
    """One REFUSALS call with null data pointers.  `workspace`: an address that is not null, with a size claimed beyond any
    need, so that no refusal is the workspace's; it also stands in where a null pointer would be refused before the shape is
    looked at (qkt_output of the materialising form).
    data: the address given for EVERY data pointer of the newer entry points (prompt, ALiBi, soft-cap, rotary, sink logits)
    instead of null (the sink logits themselves are `workspace` or, where the row says they are not given, null).
    Those launchers answer MLI_ERR_BAD_ARG for a null pointer too, so with null pointers a refusal says nothing of where the
    shape rule stands; with `data` set the pointer checks pass and only the shape rule can refuse.  Used WITHOUT a GPU only
    (tests/test_shape_limits_cpu.py): had the rule let the shape through, the launch fails there with a HIP error, which is
    not MLI_ERR_BAD_ARG.  On the device the pointers stay null, so that nothing can ever follow them."""
    tail = (workspace, workspace_bytes, stream)
    if entry == "scan":
        B, S, D, elem, phases = args
        return lib.mli_decode_scan_paged(None, None, None, None if phases & 4 else workspace, None, B, S, D, elem, phases, *tail)
    if entry == "contiguous":
        return lib.mli_decode_scan_contiguous(None, None, None, None, None, *args, *tail)
    if entry == "contiguous_kt4":
        return lib.mli_decode_scan_contiguous(None, (workspace or 4096) + 4, None, None, None, *args, *tail)
    if entry in ("qkt_paged", "qkt_paged_bf16", "qkt"):
        return getattr(lib, "mli_" + entry)(None, None, None, None, *args, stream)
    # the newer entry points: `workspace` also stands in for the slopes, the rotary table and token_logprob, which are
    # refused when null before the shape is looked at and are never followed by a launcher
    d = data
    if entry == "prompt":
        return lib.mli_prompt_scan_paged(*(d,) * 7, *args, stream)
    if entry == "prompt_softcap":
        return lib.mli_prompt_scan_paged_softcap(*(d,) * 7, *args, stream)
    if entry == "prompt_project_q":
        return lib.mli_prompt_project_q(*(d,) * 8, *args, stream)
    if entry == "prompt_logprobs":
        return lib.mli_paged_prompt_logprobs(*(d,) * 8, workspace, None, None, *args, 0, workspace, workspace_bytes, stream)
    if entry == "alibi":
        *shape, slopes, elem = args
        return lib.mli_decode_scan_paged_alibi(d, d, d, d, *shape, workspace if slopes else None, elem, *tail)
    if entry == "softcap":
        return lib.mli_decode_scan_paged_softcap(d, d, d, d, *args, *tail)
    if entry == "latest_rope":
        B, S, D, H, elem = args
        return lib.mli_get_latest_k_q_v_paged_rope(*(d,) * 6, B, S, D, H, workspace, elem, stream)
    if entry == "fill_rope":
        B, S, D, n_new, H, elem = args
        return lib.mli_fill_new_k_v_cache_paged_rope(*(d,) * 5, B, S, D, n_new, H, workspace, elem, stream)
    if entry == "prefill_rope":
        B, S, D, n_new, W, K, H, elem = args
        return lib.mli_paged_prefill_rope(*(d,) * 8, B, S, D, n_new, W, K, H, workspace, elem, stream)
    if entry == "lean_rope":
        B, S, D, n_new, H, Hkv, W, K, elem = args
        return lib.mli_paged_attention_lean_rope(*(d,) * 8, B, S, D, n_new, H, Hkv, W, K, None, workspace, elem, *tail)
    # the sink-logit entry points: `data` for every pointer but the logits, which are `workspace` (never followed) or null
    if entry in ("sink_logits", "lean_sink_logits"):
        *shape, given, elem = args
        B, S, D, *heads = shape
        z = workspace if given else None
        if entry == "sink_logits":
            return lib.mli_decode_scan_paged_sink_logits(d, d, d, d, B, S, D, *heads, z, elem, *tail)
        return lib.mli_paged_attention_lean_sink_logits(*(d,) * 5, None, d, d, B, S, D, 0, *heads, z, None, elem, *tail)
    if entry == "prompt_sink_logits":
        *shape, given, elem = args
        return lib.mli_prompt_scan_paged_sink_logits(*(d,) * 7, *shape, workspace if given else None, elem, stream)
    if entry == "prompt_logprobs_sink_logits":
        *shape, given, elem = args
        return lib.mli_paged_prompt_logprobs_sink_logits(*(d,) * 8, workspace, None, None, *shape, workspace if given else None, elem,
                                                         0, workspace, workspace_bytes, stream)
    name = {"heads": "mli_decode_scan_paged_heads", "window": "mli_decode_scan_paged_window",
            "sinks": "mli_decode_scan_paged_sinks", "gqa": "mli_decode_scan_paged_gqa"}[entry]
    return getattr(lib, name)(None, None, None, None, *args, *tail)


def rule_line(limit):
    """(line number, line) of the one line of the file that holds the rule's text"""
    path, text = limit.rule
    with open(os.path.join(ROOT, path)) as f:
        hits = [(i + 1, line) for i, line in enumerate(f.read().split("\n")) if text in line]
    assert len(hits) == 1, f"{limit.name}: `{text}` stands on {len(hits)} lines of {path}"
    return hits[0]


def markdown_rows():
    """DESIGN 6's table from LIMITS, without the measured column (tests/test_shape_limits_cpu.py holds DESIGN.md to it)"""
    return [f"| {l.name} | `{l.rule[0].split('/')[-1]}`: `{l.rule[1]}` | {l.near} | {l.far} | {l.near_outcome} | {l.far_outcome} |"
            for l in LIMITS]


# ---- two limits that reading shows unreachable, as arithmetic ------------------------------------------------------------------
def stream_triples_bound(W, dyn_pct, granule):
    """attention_stream.hip, stream_triples_bound: the triples a row of W pages can have under the split"""
    s_min = max(1, ST_MIN_PAGES * (100 - dyn_pct) // 100)
    piece = min(s_min, granule) if dyn_pct > 0 else s_min
    return W // piece + 4


def softmax_v_lds_bytes(ct, D, vec):
    """attention_scan.hip, launch_softmax_v_impl: probabilities of the item | page pointers | the waves' slice sums"""
    nj = min(2, -(-(D // vec) // 64))
    return ct * 4 + ct // PAGE * 8 + 4 * 64 * nj * vec * 4
