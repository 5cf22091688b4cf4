"""Rotary position embeddings for the tests: the float64 model of the rotated projection / fill, its judge, a
numpy stand-in of the epilogue with one defect at a time, and the engine replay with rotated q and K.

The operation (include/mli_kernels.h, the ROPE block): columns 2i and 2i + 1 of every head (hd = D / H) are pair i; for the
token at absolute slot s of its row and (c, sn) = table[s][i]

    y'[2i] = a c - b sn        y'[2i + 1] = b c + a sn        (a, b) = (y[2i], y[2i + 1])

on K (before its one rounding to the page's element type) and on q; V and x are untouched.  The model rotates
gemm_model.product's float64 K and q by the fp32 table's values TAKEN AS EXACT: the table is an input, not something a
kernel computes.

THE BOUND of a rotated element, derived, never measured.  gemm_model holds an un-rotated fp32 element to
|y~ - y| <= T = f64_model.tolerance(E_oracle) * scale(row).  The kernel rotates its own accumulators a~, b~:
    |(a~ c - b~ sn) - (a c - b sn)| <= |c| |a~ - a| + |sn| |b~ - b| <= (|c| + |sn|) T
and evaluates the rotation in fp32 as fma(+-other, sn, fl(own * c)): the product rounds once (<= 2^-24 |own c|), the fma
once (<= 2^-24 |result| <= 2^-24 (|own c| + |other sn|) (1 + 2^-24)); with |c|, |sn| <= 1 that is below
2 * 2^-24 (|a~| + |b~|), and 3 * 2^-24 (|a| + |b|) leaves the third unit for a~, b~ in place of a, b.  So
    |y'~ - y'| <= (|c| + |sn|) T + 3 * 2^-24 (|a| + |b|)
and `rotated_error` returns, per row, max_j (|g_j - y'_j| - half_step_j - 3 * 2^-24 (|a| + |b|)_j) / ((|c| + |sn|)_j scale):
the figure Figures.check holds to the same tolerance(E_oracle) as every un-rotated element.  |c| + |sn| >= 1 for any entry
on the unit circle; an entry is used as it is given, on the circle or not.  half_step is gemm_model.stored_error's term for K that leaves
rounded to bf16 / fp8 (gemm_model.half_step, 0 for fp32), taken off before the division exactly as there.

TEST INFRASTRUCTURE: never used by the product."""
import contextlib
import math
from dataclasses import dataclass

import numpy as np

import gemm_model as gm
import replay_model as rm

U = 2.0 ** -24


# ---- tables ----------------------------------------------------------------------------------------------------------------------
def standard_table(n_sequence, head_dim, theta=10000.0):
    """An independent restatement of mli_rope_table in numpy float64: float32 [S, hd / 2, 2] of (cos, sin)(s theta^(-2i/hd))."""
    i = np.arange(head_dim // 2, dtype=np.float64)
    inv = np.power(np.float64(theta), -2.0 * i / head_dim)
    ang = np.arange(n_sequence, dtype=np.float64)[:, None] * inv[None, :]
    return np.stack([np.cos(ang), np.sin(ang)], axis=-1).astype(np.float32)


def identity_table(n_sequence, head_dim):
    t = np.zeros((n_sequence, head_dim // 2, 2), np.float32)
    t[..., 0] = 1.0
    return t


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _pairing(D, hd, pairing):
    """(partner column of every column, whether the column is the pair's second, frequency index of the column)"""
    n = np.arange(D)
    j = n % hd
    if pairing == "interleaved":
        return n ^ 1, (n & 1) == 1, j // 2
    if pairing == "shifted":          # pairs (2i + 1, 2i + 2), wrapping inside the row
        second = (n & 1) == 0
        return np.where(second, n - 1, n + 1) % D, second, ((j + 1) % hd) // 2
    if pairing == "half_split":       # HF rotate_half: column j pairs with j + hd / 2
        second = j >= hd // 2
        return np.where(second, n - hd // 2, n + hd // 2), second, j % (hd // 2)
    if pairing == "freq_n2":          # the right pairs with the frequency index n / 2: right in the first head only
        return n ^ 1, (n & 1) == 1, n // 2
    raise ValueError(pairing)


def rotate(y, slots, table, n_heads, pairing="interleaved", sign=1.0, dtype=np.float64):
    """y [R, D] rotated row by row by table[slots[r]].  dtype float32 = the epilogue's own arithmetic (one product rounding, one
    fma rounding, the fma evaluated in float64 and rounded once).  A frequency index beyond hd / 2 (the freq_n2 defect) reads
    on in the table's memory, as a kernel would."""
    y = np.asarray(y)
    R, D = y.shape
    if R == 0:
        return np.zeros((0, D), dtype)
    hd = D // n_heads
    partner, second, fi = _pairing(D, hd, pairing)
    flat = np.asarray(table, np.float32).reshape(-1, 2)
    idx = np.minimum(np.asarray(slots, np.int64)[:, None] * (hd // 2) + fi[None, :], len(flat) - 1)
    c, sn = flat[idx, 0].astype(np.float64), flat[idx, 1].astype(np.float64) * sign
    own, other = y.astype(np.float64), y[:, partner].astype(np.float64)
    other = np.where(second[None, :], other, -other)
    if dtype == np.float32:
        t = (y.astype(np.float32) * flat[idx, 0]).astype(np.float64)     # fl(own * c)
        return (other * sn + t).astype(np.float32)                       # fma: exact in float64 (24 + 24 bits), one rounding
    return own * c + other * sn


def rotation_terms(y, slots, table, n_heads):
    """(|c| + |sn| per element, |a| + |b| per element) of the bound above, for the float64 un-rotated y"""
    y = np.asarray(y, np.float64)
    R, D = y.shape
    hd = D // n_heads
    fi = (np.arange(D) % hd) // 2
    t = np.asarray(table, np.float32).astype(np.float64)[np.asarray(slots, np.int64)][:, fi] if R else np.zeros((0, D, 2))
    pair = np.abs(y) + np.abs(y[:, np.arange(D) ^ 1])
    return np.abs(t[..., 0]) + np.abs(t[..., 1]), pair


def rotated_error(got_values, want_rot, gain, pair, scale, fmt):
    """The per-row figure of the module docstring; a non-finite value on either side is an infinite error."""
    g = np.asarray(got_values).astype(np.float64)
    y = np.clip(want_rot, -448.0, 448.0) if fmt == "fp8" else np.asarray(want_rot, np.float64)
    err = np.zeros(len(y), np.float64)
    for r in range(len(y)):
        if not (np.isfinite(g[r]).all() and np.isfinite(y[r]).all()):
            err[r] = np.inf
            continue
        half = 0.0 if fmt == "f32" else gm.half_step(np.maximum(np.abs(g[r]), np.abs(y[r])), fmt)
        over = (np.abs(g[r] - y[r]) - half - 3.0 * U * pair[r]) / gain[r]
        err[r] = max(float(over.max()), 0.0) / scale[r]
    return err


def page_dead(page, n, window, n_sink):
    """page_live.hpp: page i of a row of n tokens is dead iff ceil(K / 16) <= i < max(0, n - W) / 16"""
    return -(-n_sink // 16) <= page < max(0, n - window) // 16


class Expect(gm.Expect):
    """gemm_model.Expect plus the rotated K and q: slots = the absolute slot of every written row (gemm_model's rows are
    (batch row, token): L - 1 for a latest case, the token for a fill)."""

    def __init__(self, oracle, c, mode, table, n_heads, window=0, n_sink=0):
        super().__init__(oracle, c, mode)
        self.table, self.n_heads = np.asarray(table, np.float32), n_heads
        if window and mode != "latest":   # the windowed prefill writes a row's LIVE tokens only (page_live.hpp)
            keep = np.array([not page_dead(s // 16, int(c.L[b]), window, n_sink) for b, s in self.rows], bool)
            self.rows = [r for r, k in zip(self.rows, keep) if k]
            self.x = self.x[keep]
            for d in (self.want, self.scale, self.oracle):
                for n in d:
                    d[n] = d[n][keep] if d[n] is not None else None
        self.slots = np.array([r[1] for r in self.rows], np.int64)
        self.rot, self.gain, self.pair = {}, {}, {}
        for n in ("wk", "wq"):
            if n in self.want:
                self.rot[n] = rotate(self.want[n], self.slots, table, n_heads)
                self.gain[n], self.pair[n] = rotation_terms(self.want[n], self.slots, table, n_heads)


def judge(fig, c, e, after, q_after, also=()):
    """gemm_model.judge for a *_rope call on pages: K and q against the rotated model under the derived bound, V under
    gemm_model's, x of a prefill bit-exact, every byte the contract does not write unchanged, nothing non-finite."""
    fmt, rows = c.fmt, e.rows
    values = gm.decode(after["pool"], fmt)
    fig.require(np.isfinite(values).all(), "non-finite value in the page pool")
    written = np.zeros(c.pool.size, bool)
    got = {"wk": np.zeros((0, c.Dout)), "wv": np.zeros((0, c.Dout))}
    if rows:
        for n, seg in (("wk", 1), ("wv", 2)):
            off = gm._slot_offsets(c, rows, seg)
            got[n] = values[off]
            written[off.ravel()] = True
        if e.embed:
            off = gm._slot_offsets(c, rows, 0)
            written[off.ravel()] = True
            same = gm.raw_bits(after["pool"], fmt)[off] == gm.raw_bits(gm.encode(e.x, fmt), fmt)
            fig.require(same.all(), f"x of the prefill: {int((~same).sum())} elements differ from emb[tok] + wpe[s] rounded once")
    if len(also):
        for seg in (1, 2):
            written[gm._slot_offsets(c, list(also), seg).ravel()] = True
    same = gm.raw_bits(after["pool"], fmt)[~written] == gm.raw_bits(c.pool, fmt)[~written]
    fig.require(same.all(), f"{int((~same).sum())} pool elements outside the written slots changed")
    e_k = gm.fp32_error(e.oracle["wk"], e.want["wk"], e.scale["wk"])
    fig.check(f"K rotated ({fmt})", rotated_error(got["wk"], e.rot["wk"], e.gain["wk"], e.pair["wk"], e.scale["wk"], fmt), e_k, c.Din)
    e_v = gm.fp32_error(e.oracle["wv"], e.want["wv"], e.scale["wv"])
    fig.check(f"V ({fmt})", gm.stored_error(got["wv"], e.want["wv"], e.scale["wv"], fmt), e_v, c.Din)
    if q_after is not None:
        fig.require(np.isfinite(q_after).all(), "non-finite value in q_output")
        live = np.array([r[0] for r in rows], np.int64)
        empty = np.ones(c.B, bool)
        empty[live] = False
        same = q_after.view(np.uint32)[empty] == c.q.view(np.uint32)[empty]
        fig.require(same.all(), "q_output of an empty row was written")
        fig.check("q rotated", rotated_error(q_after[live], e.rot["wq"], e.gain["wq"], e.pair["wq"], e.scale["wq"], "f32"),
                  gm.fp32_error(e.oracle["wq"], e.want["wq"], e.scale["wq"]), c.Din)
    return fig


# ---- the epilogue restated in numpy, with one defect at a time ---------------------------------------------------------------------
DEFECTS = ("sign of sn flipped", "pairs (2i + 1, 2i + 2)", "half-split pairing", "frequency index n / 2", "position L",
           "flat-list index as position", "live index as position", "V rotated as well", "q not rotated",
           "rotation after the rounding")


def live_index(s, L, window, n_sink):
    """the index of slot s among the live tokens of a row of L tokens (page_live.hpp): slots of dead pages are not counted"""
    PAGE = 16
    lo = max(0, L - window)
    p0, ps = lo // PAGE, -(-n_sink // PAGE)
    skip = max(0, p0 - ps)
    return s if s < PAGE * ps or skip == 0 else s - PAGE * skip


def restate(c, e, defect=None, window=0, n_sink=0):
    """The call of case c as a kernel with the rotation in its epilogue would run it, in numpy float32: x @ w (numpy's own
    summation order), the rotation in the epilogue's arithmetic, one rounding.  Returns (after, q_after) in judge's form."""
    rows, table, H = list(e.rows), e.table, e.n_heads
    x = e.x
    slots = e.slots.copy()
    if defect == "position L":
        slots = np.minimum(slots + 1, len(table) - 1)
    elif defect == "flat-list index as position":
        slots = np.arange(len(rows), dtype=np.int64) % len(table)
    elif defect == "live index as position":
        slots = np.array([live_index(s, int(c.L[b]), window, n_sink) for b, s in rows], np.int64)
    kw = {"sign of sn flipped": dict(sign=-1.0), "pairs (2i + 1, 2i + 2)": dict(pairing="shifted"),
          "half-split pairing": dict(pairing="half_split"), "frequency index n / 2": dict(pairing="freq_n2")}.get(defect, {})
    pool = c.pool.copy()
    y = {n: (np.asarray(x, np.float32) @ np.asarray(c.w[n], np.float32)).astype(np.float32) for n in e.want}
    k = y["wk"]
    if defect == "rotation after the rounding":
        k = rotate(gm.round_to(k, c.fmt), slots, table, H, dtype=np.float32)
    else:
        k = rotate(k, slots, table, H, dtype=np.float32, **kw)
    v = rotate(y["wv"], slots, table, H, dtype=np.float32) if defect == "V rotated as well" else y["wv"]
    if rows:
        pool[gm._slot_offsets(c, rows, 1)] = gm.encode(k, c.fmt)
        pool[gm._slot_offsets(c, rows, 2)] = gm.encode(v, c.fmt)
        if e.embed:
            pool[gm._slot_offsets(c, rows, 0)] = gm.encode(x, c.fmt)
    q_after = None
    if e.mode == "latest":
        q_after = c.q.copy()
        if rows:
            q = y["wq"] if defect == "q not rotated" else rotate(y["wq"], slots, table, H, dtype=np.float32, **kw)
            q_after[np.array([r[0] for r in rows], np.int64)] = q
    return {"pool": pool}, q_after


# ---- the engine replay with rotated q and stored K -----------------------------------------------------------------------------------
@dataclass(frozen=True)
class RopeSpec(rm.Spec):
    table: bytes = b""     # the fp32 table's bytes (hashable: the spec keys replay_model's cache)

    def name(self):
        return super().name() + " rope"

    def values(self, emb_dim):
        hd = emb_dim // self.n_heads
        return np.frombuffer(self.table, np.float32).reshape(-1, hd // 2, 2)


def rope_spec(spec, table):
    """the RopeSpec of a replay_model.Spec and a float32 table [S, hd / 2, 2]"""
    return RopeSpec(spec.store, spec.n_heads, spec.window, spec.n_sink, spec.flips, np.ascontiguousarray(table, np.float32).tobytes())


def logits_from_state(x, K, V, wq, emb, mask, n_heads, table, rows, dtype=np.float64):
    """replay_model.logits_from_state with q of position i rotated by table[i] (K arrives rotated by its slot)"""
    x, K, V, wq, emb = (np.asarray(a).astype(dtype) for a in (x, K, V, wq, emb))
    rows = np.asarray(rows)
    x, mask = x[rows], mask[rows]
    D = x.shape[1]
    hd = D // n_heads
    q = rotate(x @ wq, rows, table, n_heads, dtype=dtype).astype(dtype)
    out = np.empty((x.shape[0], D), dtype)
    scale = dtype(1.0 / math.sqrt(hd))
    for h in range(n_heads):
        sl = slice(h * hd, (h + 1) * hd)
        s = np.where(mask, (q[:, sl] @ K[:, sl].T) * scale, dtype(-np.inf))
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p = p / p.sum(axis=1, keepdims=True, dtype=dtype)
        out[:, sl] = p @ V[:, sl]
    return out @ emb.T


def project_rotated(x, w, store, emb_dim, table, n_heads):
    """replay_model.project for K under the rotation: rotate, THEN store.  The ambiguity bound carries through the rotation:
    an fp32 accumulation error of at most beta_j per un-rotated element moves the rotated one by at most
    |c| beta_own + |sn| beta_partner (plus the epilogue's own 3 * 2^-24 (|a| + |b|))."""
    slots = np.arange(x.shape[0])
    y = x @ w
    v = rotate(y, slots, table, n_heads)
    if store == "f32":
        return v, v, np.zeros(v.shape, bool)
    near, other = rm.store_neighbours(v, store)
    beta = emb_dim * U * (np.abs(x) @ np.abs(w))
    gain_c, _ = rotation_terms(y, slots, table, n_heads)      # |c| + |sn| >= either factor
    D = y.shape[1]
    bound = gain_c * np.maximum(beta, beta[:, np.arange(D) ^ 1]) + 3.0 * U * (np.abs(y) + np.abs(y[:, np.arange(D) ^ 1]))
    amb = (np.abs(v - 0.5 * (near + other)) <= bound) & (other != near)
    return near, other, amb


class RopeReplay(rm.Replay):
    """replay_model.Replay with the stored K rotated by its slot and q by its position"""

    def __init__(self, model, tokens, spec, rows=None):
        n, D = len(tokens), np.shape(model["wk"])[0]
        w = rm.weights(model, spec.store)
        self.spec, self.wq = spec, w["wq"]
        self.table = spec.values(D)
        self.emb = np.asarray(model["emb_table"], np.float32).astype(np.float64)
        self.x = rm.embed(model, tokens, spec.store)
        self.K, self.K_other, self.K_amb = project_rotated(self.x, w["wk"], spec.store, D, self.table, spec.n_heads)
        self.V, self.V_other, self.V_amb = rm.project(self.x, w["wv"], spec.store, D)
        self.mask = rm.causal_mask(n, spec.window, spec.n_sink)
        self.rows = np.arange(n) if rows is None else np.asarray(rows)
        self.logits = self._logits(self.K, self.V)

    def _logits(self, K, V, dtype=np.float64):
        return logits_from_state(self.x, K, V, self.wq, self.emb, self.mask, self.spec.n_heads, self.table, self.rows, dtype)


@contextlib.contextmanager
def _rope_forward():
    """replay_model's judges with RopeReplay as their forward, as alibi_model._alibi_forward: the module global `Replay` is
    swapped for the duration of one audit (one thread; the judge's cache is keyed by the spec, table included)."""
    plain = rm.Replay
    rm.Replay = RopeReplay
    try:
        yield
    finally:
        rm.Replay = plain


def audit(model, items, finished, spec, n_sequence, **kw):
    """replay_model.audit under a RopeSpec; its rules, MASK_CAP included, are replay_model's"""
    assert isinstance(spec, RopeSpec) and len(spec.table) == 4 * n_sequence * (np.shape(model["wk"])[0] // spec.n_heads)
    with _rope_forward():
        return rm.audit(model, items, finished, spec, n_sequence, **kw)


def generate(model, prompt, spec, n_sequence, wrong_table=None):
    """Decode one item greedily on the float64 rotated forward (the choice on the float32-rounded logits, as the CPU engines
    choose); wrong_table: the table the generator uses instead of the spec's (a wrong engine for the audit to reject)."""
    import sampling_ref as sr
    used = spec if wrong_table is None else rope_spec(spec, wrong_table)
    toks = [int(t) for t in prompt]
    while True:
        rep = RopeReplay(model, toks, used, rows=[len(toks) - 1])
        tok = int(sr.greedy(rep.logits[0].astype(np.float32)))
        toks.append(tok)
        if len(toks) >= n_sequence or tok == rm.EOF:
            return np.asarray(toks, np.int32)
