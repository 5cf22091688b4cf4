"""Float64 model, metrics and judges of the dense products (GEMM block): the decode projection x.[Wk|Wq|Wv], the
prefill fill X.[Wk|Wv] and the logits att.emb^T.  numpy only; shared by tests/test_gemm_model_cpu.py (which proves that the
comparison can fail) and tests/test_gemm_edges_gpu.py (which runs the kernels through it).

Everything a test compares is PER ROW and normalised by the row's condition scale max_j sum_i |x_i w_ij| (f64_model's
projection metric).  fp32 results are held to f64_model.tolerance(E_oracle) and to the ceiling K * 2^-24 no fp32 summation
order can exceed; K / V that leave a kernel rounded to bf16 / fp8 go through stored_error, which takes the format's half
step off every element first, so the same tolerance applies to "an fp32 value within tol * scale, rounded once"."""
import numpy as np

import f64_model as fm
from helpers import (PAGE, bf16_bits, build_page_pool, fp8_bits, fp8_decode, gather_rows_from_pool, rand_f)

ESIZE = {"f32": 4, "bf16": 2, "fp8": 1}
ELEM = {"f32": 0, "bf16": 1, "fp8": 2}
BITS = {"f32": np.uint32, "bf16": np.uint16, "fp8": np.uint8}


# ---- number formats ------------------------------------------------------------------------------------------------
def encode(values, fmt):
    """float32 values -> what memory holds (float32 / bf16 bit patterns / e4m3 byte codes), rounded to nearest even."""
    v = np.ascontiguousarray(values, np.float32)
    return v.copy() if fmt == "f32" else (bf16_bits(v) if fmt == "bf16" else fp8_bits(v)).reshape(v.shape)


def decode(stored, fmt):
    if fmt == "f32":
        return np.asarray(stored, np.float32)
    if fmt == "bf16":
        return (np.asarray(stored, np.uint16).astype(np.uint32) << 16).view(np.float32)
    return fp8_decode(stored).reshape(np.shape(stored))


def round_to(values, fmt):
    return decode(encode(values, fmt), fmt)


def raw_bits(stored, fmt):
    """The bytes of a stored array as unsigned integers (NaN-proof bit comparison)."""
    return np.ascontiguousarray(stored).view(BITS[fmt])


def half_step(v, fmt):
    """Half the spacing of the format at magnitude |v|: bf16 2^(floor(log2|v|) - 8), e4m3 2^(max(floor(log2|v|), -6) - 4)."""
    a = np.abs(np.asarray(v, np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - 8) if fmt == "bf16" else 2.0 ** (np.maximum(e, -6) - 4)


# ---- the model -----------------------------------------------------------------------------------------------------
def product(x, w):
    """(float64 x @ w, per-row condition scale max_j sum_i |x_i w_ij|)."""
    x64, w64 = fm._f64(x), fm._f64(w)
    if x64.shape[0] == 0:
        return np.zeros((0, w64.shape[1])), np.zeros(0)
    return x64 @ w64, (np.abs(x64) @ np.abs(w64)).max(axis=1)


def fill_rows(new_rows, lengths):
    """The (row, token) pairs a fill writes, in the order of its flat list: every s < L of every new row."""
    return [(int(b), s) for b in new_rows for s in range(int(lengths[int(b)]))]


def project_fill(x, new_rows, lengths, wk, wv):
    """K and V (float64 [n_pairs, Dout]) of every token s < L of every new row of x [B, S, Din], in fill_rows order, and
    the per-(row, token) condition scales of the two products."""
    rows = fill_rows(new_rows, lengths)
    xs = np.zeros((0, x.shape[2])) if not rows else x[[r[0] for r in rows], [r[1] for r in rows]]
    k, ks = product(xs, wk)
    v, vs = product(xs, wv)
    return k, v, ks, vs


def logits(att, emb):
    """(float64 att @ emb.T, per-row scale max_v sum_i |a_i e_vi|)."""
    return product(att, np.asarray(emb).T)


# ---- metrics -------------------------------------------------------------------------------------------------------
def fp32_error(got, want64, scale):
    """f64_model.projection_error over a flat list of rows (every row is live)."""
    return fm.projection_error(got, want64, np.ones(len(want64), np.int64), scale)


def stored_error(got_values, want64, scale, fmt):
    """Per row max_j (|g_j - y_j| - half_step(max(|g_j|, |y_j|))) / scale, clipped below at 0; y is clipped to +-448 for
    fp8 (the store saturates); a non-finite value on either side is an infinite error.  fmt f32 = fp32_error."""
    if fmt == "f32":
        return fp32_error(got_values, want64, scale)
    g = np.asarray(got_values).astype(np.float64)
    y = np.clip(want64, -448.0, 448.0) if fmt == "fp8" else np.asarray(want64, np.float64)
    err = np.zeros(len(y), np.float64)
    for r in range(len(y)):
        if not (np.isfinite(g[r]).all() and np.isfinite(y[r]).all()):
            err[r] = np.inf
            continue
        over = np.abs(g[r] - y[r]) - half_step(np.maximum(np.abs(g[r]), np.abs(y[r])), fmt)
        err[r] = max(float(over.max()), 0.0) / scale[r]
    return err


def ceiling(k_dim):
    """What no fp32 accumulation of k_dim products can exceed in the normalised metric, in any order."""
    return k_dim * 2.0 ** -24


def oracle_product(oracle, x, w):
    """The CPU oracle's evaluation of x @ w: oracle_gemm_transpose runs, per output element, the loop of
    oracle_get_latest_kt_q_v and oracle_fill_new_kt_v_cache (one sequential fp32 sum over k, product then add), with
    unit-stride operands -- tests/test_gemm_model_cpu.py checks that the three agree bit for bit."""
    x = np.ascontiguousarray(x, np.float32)
    if x.shape[0] == 0:
        return np.zeros((0, w.shape[1]), np.float32)
    return oracle.gemm_transpose_host(x, np.ascontiguousarray(np.asarray(w, np.float32).T))


# ---- data ----------------------------------------------------------------------------------------------------------
def draw(rng, shape, family):
    """signed: U(-1, 1); positive: the reference's U(0, 1] (no cancellation, large sums)."""
    return rand_f(rng, shape) if family == "positive" else (rng.random(shape, dtype=np.float32) * 2 - 1).astype(np.float32)


def draw_w(rng, k_dim, n_dim, family):
    w = draw(rng, (k_dim, n_dim), family)
    return w if family == "positive" else (w * np.float32(2.0 / np.sqrt(k_dim))).astype(np.float32)


FILL_LENGTHS = [63, 17, 0, 65, 1, 64, 15, 16]   # flat list: 0..62 | 63..79 (crosses tile 0 / 1) | - | 80..144 (crosses 1 / 2) ...


def edge_lengths(n_batch, n_sequence, rng, empty_every=4):
    """Lengths of a latest case: 0, 1, 16, 17 and S - 1 where B allows, random elsewhere, every empty_every-th row empty."""
    L = rng.integers(1, n_sequence, size=n_batch).astype(np.int32)
    if empty_every and n_batch > 1:
        L[::empty_every] = 0
    edges = [n_sequence - 1, 17, 16, 1]
    live = [b for b in range(n_batch) if L[b] > 0] if n_batch > 1 else [0]
    for b, e in zip(live, edges):
        L[b] = e
    return L


def fill_layout(n_batch, n_sequence, rng):
    """(lengths, new_batch_idx, n_new) of a fill case: the new rows carry FILL_LENGTHS in that order at non-monotone batch
    indices (as many as B allows), the other rows are old (random length, never written)."""
    lens = [l for l in FILL_LENGTHS if l < n_sequence][:n_batch]
    L = rng.integers(0, n_sequence, size=n_batch).astype(np.int32)
    order = rng.permutation(n_batch)[:len(lens)].astype(np.int32)
    if len(order) > 2 and (np.diff(order) > 0).all():
        order[:2] = order[1::-1]
    L[order] = lens
    new_idx = rng.integers(0, n_batch, size=n_batch).astype(np.int32)
    new_idx[:len(order)] = order
    return L, new_idx, len(order)


class Case:
    """One projection / fill / prefill case over pages (layout "paged") or the contiguous caches (layout "naive").
    Holds what memory holds BEFORE the call: stored arrays (encode) and their float32 values."""

    def __init__(self, seed, layout, fmt, family, B, S, Din, Dout, lengths, new_idx=None, n_new=0, vocab=0, saturate=False):
        rng = np.random.default_rng(seed)
        self.layout, self.fmt, self.family, self.B, self.S, self.Din, self.Dout = layout, fmt, family, B, S, Din, Dout
        self.L = np.asarray(lengths, np.int32)
        self.new_idx = np.zeros(B, np.int32) if new_idx is None else np.asarray(new_idx, np.int32)
        self.n_new = int(n_new)
        wfmt = "f32" if fmt == "f32" else "bf16"
        self.w = {n: round_to(draw_w(rng, Din, Dout, family), wfmt) for n in ("wk", "wq", "wv")}
        self.q = draw(rng, (B, Dout), family)
        if layout == "paged":
            assert Din == Dout and S % PAGE == 0
            pool, self.table = build_page_pool(rng, self.L, S, Din, spare_blocks=1)
            pool = pool if family == "positive" else (pool * 2 - 1).astype(np.float32)
            self.pool = encode(pool, fmt)
        else:
            assert fmt == "f32"
            self.inp = draw(rng, (B, S, Din), family)
            self.kt = draw(rng, (B, Dout, S), family)
            self.v = draw(rng, (B, S, Dout), family)
        if vocab:   # prefill: x = emb[tok] + wpe[s]
            self.emb = draw(rng, (vocab, Din), family)
            self.wpe = draw(rng, (S, Din), family)
            self.tok = rng.integers(0, vocab, size=(B, S)).astype(np.int32)
            if saturate:   # one vocabulary row beyond the fp8 range, used by the first new row throughout
                self.emb[3] *= np.float32(600.0)
                self.tok[int(self.new_idx[0]), :] = 3

    def x_rows(self, rows, embed):
        """float32 x of the (row, token) pairs, as the kernel reads it."""
        if not rows:
            return np.zeros((0, self.Din), np.float32)
        bb, ss = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        if embed:
            return round_to(self.emb[self.tok[bb, ss]] + self.wpe[ss], self.fmt)
        if self.layout == "paged":
            return gather_rows_from_pool(decode(self.pool, self.fmt), self.table, rows, 0, self.Din)
        return self.inp[bb, ss]


def latest_case(seed, fmt, family, B, S, D, layout="paged", Dout=None, empty_every=4):
    rng = np.random.default_rng(seed)
    return Case(seed, layout, fmt, family, B, S, D, Dout or D, edge_lengths(B, S, rng, empty_every)), "latest"


def fill_case(seed, fmt, family, B, S, D, layout="paged", Dout=None, mode="fill", saturate=False, lengths=None):
    """lengths given: every row is new with that length (the 2048 / 2049 new-row cases); else fill_layout."""
    rng = np.random.default_rng(seed)
    if lengths is None:
        L, new_idx, n_new = fill_layout(B, S, rng)
    else:
        L, new_idx, n_new = np.asarray(lengths, np.int32), rng.permutation(B).astype(np.int32), B
    return Case(seed, layout, fmt, family, B, S, D, Dout or D, L, new_idx, n_new, vocab=40 if mode == "prefill" else 0,
                saturate=saturate), mode


class Expect:
    """What a call must leave: the slots it writes, their float64 values and scales, and the oracle's fp32 values."""

    def __init__(self, oracle, c, mode):
        self.mode, self.embed = mode, mode == "prefill"
        if mode == "latest":
            self.rows = [(b, int(c.L[b]) - 1) for b in range(c.B) if c.L[b] > 0]
            names = ("wk", "wq", "wv")
        else:
            self.rows = fill_rows(c.new_idx[:c.n_new], c.L)
            names = ("wk", "wv")
        self.x = c.x_rows(self.rows, self.embed)
        self.want, self.scale, self.oracle = {}, {}, {}
        if mode == "latest":   # through f64_model.project_latest: one position per live row
            live = np.array([r[0] for r in self.rows], np.int64)
            q, k, v, qs, ks, vs = fm.project_latest(self.x[:, None, :], np.ones(len(live), np.int64), c.w["wk"], c.w["wq"], c.w["wv"])
            self.want, self.scale = {"wk": k, "wq": q, "wv": v}, {"wk": ks, "wq": qs, "wv": vs}
        else:
            x_bsd = np.zeros((c.B, c.S, c.Din), np.float32)
            if self.rows:
                x_bsd[[r[0] for r in self.rows], [r[1] for r in self.rows]] = self.x
            k, v, ks, vs = project_fill(x_bsd, c.new_idx[:c.n_new], c.L, c.w["wk"], c.w["wv"])
            self.want, self.scale = {"wk": k, "wv": v}, {"wk": ks, "wv": vs}
        for n in names:
            self.oracle[n] = oracle_product(oracle, self.x, c.w[n]) if oracle is not None else None


class Figures:
    """Collects the comparisons of one case; every figure is printed before anything is asserted."""

    def __init__(self, label):
        self.label, self.failures, self.records = label, [], []

    def check(self, what, err, e_oracle, k_dim, rule=True):
        """rule: hold to f64_model.tolerance(E_oracle); always hold to the ceiling K * 2^-24."""
        tol = fm.tolerance(e_oracle)
        worst = float(np.max(err)) if len(err) else 0.0
        e_or = float(np.max(e_oracle)) if len(e_oracle) else 0.0
        print(f"GEMM {self.label} | {what}: kernel {worst:.3e}  oracle {e_or:.3e}  tol {tol:.3e}  ceiling {ceiling(k_dim):.3e}"
              f"{'' if rule else '  (ceiling only)'}")
        self.records.append((what, worst, e_or, tol))
        bound = min(tol, ceiling(k_dim)) if rule else ceiling(k_dim)
        if not worst <= bound:
            bad = np.nonzero(~(np.asarray(err) <= bound))[0]
            self.failures.append(f"{self.label} {what}: {worst:.3e} > {bound:.3e} (oracle {e_or:.3e}) in rows {bad[:8].tolist()}")
        return tol

    def require(self, ok, message):
        if not ok:
            self.failures.append(f"{self.label} {message}")

    def done(self):
        assert not self.failures, "\n".join(self.failures)


def _slot_offsets(c, rows, seg):
    bb, ss = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    base = c.table[bb, ss // PAGE] + (ss % PAGE) * 3 * c.Din + seg * c.Din
    return (base[:, None] + np.arange(c.Din)[None, :])


def judge(fig, c, e, after, q_after, rule=True, also=()):
    """The three assertions of every case on what a call left behind.  after: {"pool": stored} (paged) or {"kt": ..,
    "v": ..} plus "inp" for a prefill (naive); q_after: float32 [B, Dout] or None (fill).
    also: (row, token) slots whose K / V another step of the same call writes (a composition: judged by its own Expect).
    (a) every written K / V / q within tolerance; a prefill's x bit-exact; (b) every byte the contract does not write
    bit-identical to before; (c) nothing non-finite anywhere."""
    fmt, rows = c.fmt, e.rows
    got = {}
    if c.layout == "paged":
        values = decode(after["pool"], fmt)
        fig.require(np.isfinite(values).all(), "non-finite value in the page pool")
        written = np.zeros(c.pool.size, bool)
        if rows:
            for n, seg in (("wk", 1), ("wv", 2)):
                off = _slot_offsets(c, rows, seg)
                got[n] = values[off]
                written[off.ravel()] = True
            if e.embed:
                off = _slot_offsets(c, rows, 0)
                written[off.ravel()] = True
                same = raw_bits(after["pool"], fmt)[off] == raw_bits(encode(e.x, fmt), fmt)
                fig.require(same.all(), f"x of the prefill: {int((~same).sum())} elements differ from emb[tok] + wpe[s] rounded once")
        else:
            got = {"wk": np.zeros((0, c.Dout)), "wv": np.zeros((0, c.Dout))}
        if len(also):
            for seg in (1, 2):
                written[_slot_offsets(c, list(also), seg).ravel()] = True
        same = raw_bits(after["pool"], fmt)[~written] == raw_bits(c.pool, fmt)[~written]
        fig.require(same.all(), f"{int((~same).sum())} pool elements outside the written slots changed")
    else:
        bb, ss = (np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64))
        for name, before, index in (("kt", c.kt, lambda a: a[bb, :, ss]), ("v", c.v, lambda a: a[bb, ss])):
            a = after[name]
            fig.require(np.isfinite(a).all(), f"non-finite value in {name}_cache")
            mask = np.zeros(a.shape, bool)
            if rows:
                if name == "kt":
                    mask[bb, :, ss] = True
                else:
                    mask[bb, ss] = True
            got["wk" if name == "kt" else "wv"] = index(a) if rows else np.zeros((0, c.Dout))
            same = a.view(np.uint32)[~mask] == before.view(np.uint32)[~mask]
            fig.require(same.all(), f"{int((~same).sum())} {name}_cache elements outside the written slots changed")
        if "inp" in after:
            mask = np.zeros(c.inp.shape, bool)
            if rows:
                mask[bb, ss] = True
                same = after["inp"][bb, ss].view(np.uint32) == e.x.view(np.uint32)
                fig.require(same.all(), "x of the prefill differs from emb[tok] + wpe[s]")
            same = after["inp"].view(np.uint32)[~mask] == c.inp.view(np.uint32)[~mask]
            fig.require(same.all(), f"{int((~same).sum())} inp_embedding elements outside the new rows changed")
    for n in ("wk", "wv"):
        e_or = fp32_error(e.oracle[n], e.want[n], e.scale[n])
        tol = fig.check(f"{'K' if n == 'wk' else 'V'} ({fmt})", stored_error(got[n], e.want[n], e.scale[n], fmt), e_or, c.Din, rule)
        if fmt != "f32":   # the oracle's own values, rounded once, stay inside the bound they set
            e_st = stored_error(round_to(e.oracle[n], fmt), e.want[n], e.scale[n], fmt)
            fig.require(float(np.max(e_st, initial=0.0)) <= tol, f"oracle {n} rounded to {fmt} misses its own bound")
    if q_after is not None:
        fig.require(np.isfinite(q_after).all(), "non-finite value in q_output")
        live = np.array([r[0] for r in rows], np.int64)
        empty = np.ones(c.B, bool)
        empty[live] = False
        same = q_after.view(np.uint32)[empty] == c.q.view(np.uint32)[empty]
        fig.require(same.all(), "q_output of an empty row was written")
        fig.check("q_output", fp32_error(q_after[live], e.want["wq"], e.scale["wq"]),
                  fp32_error(e.oracle["wq"], e.want["wq"], e.scale["wq"]), c.Din, rule)
    return fig


# ---- logits and the greedy head --------------------------------------------------------------------------------------
class LogitsCase:
    def __init__(self, seed, family, B, V, D, S=32, finish=False):
        rng = np.random.default_rng(seed)
        self.family, self.B, self.V, self.D, self.S = family, B, V, D, S
        self.att = draw(rng, (B, D), family)
        self.emb = draw(rng, (V, D), family) if family == "positive" else draw_w(rng, V, D, "signed") * np.float32(np.sqrt(V / D))
        self.emb = np.ascontiguousarray(self.emb, np.float32)
        if V >= 4:   # an exact tie: a duplicated row, and batch rows that point at it -- the lower index must win
            self.emb[V - 1] = self.emb[1]
            point = self.emb[1] - self.emb.mean(axis=0) if family == "positive" else self.emb[1]   # (U(0,1] rows all point alike)
            self.att[::7] = point * np.float32(3.0)
        self.wpe = draw(rng, (S, D), family)
        self.inp = draw(rng, (B, S, D), family)
        self.L = rng.integers(1, S - 2, size=B).astype(np.int32)
        if finish:   # every live row ends on its length: the head picks a token and writes no next embedding
            self.L[:] = S - 1
        if B > 2:
            self.L[2] = 0
        self.score0 = draw(rng, (B, V), family)


def judge_logits(fig, oracle, c, score, tokens, tokens_unfused=None):
    """emb_score through the projection metric; the fused head's token = the float64 argmax (lowest index among exact
    duplicates of the winning row) wherever the float64 top-two gap exceeds 2 tol scale, within that gap of the maximum
    elsewhere; at most 1 % of the rows may fall to the weaker check (returned)."""
    want, scale = logits(c.att, c.emb)
    e_or = fp32_error(oracle_product(oracle, c.att, c.emb.T), want, scale)
    fig.require(np.isfinite(score).all(), "non-finite value in emb_score")
    tol = fig.check("emb_score", fp32_error(score, want, scale), e_or, c.D)
    _, canon = np.unique(c.emb, axis=0, return_inverse=True)
    canon = canon.ravel()
    weak = 0
    for b in range(c.B):
        if c.L[b] == 0:
            fig.require(tokens[b] == -1, f"row {b} is empty: token {tokens[b]}")
            continue
        best = int(np.argmax(want[b]))
        others = want[b][canon != canon[best]]
        gap = want[b, best] - (others.max() if len(others) else -np.inf)
        if gap > 2 * tol * scale[b]:
            fig.require(tokens[b] == best, f"row {b}: token {tokens[b]}, float64 argmax {best} (gap {gap:.3e})")
        else:
            weak += 1
            ok = 0 <= tokens[b] < c.V and want[b, best] - want[b, tokens[b]] <= 2 * tol * scale[b]
            fig.require(ok, f"row {b}: token {tokens[b]} is not within the tie gap of the maximum")
    if tokens_unfused is not None:   # launch_decoder picks from its own emb_score: exactly its first maximum
        live = c.L > 0
        fig.require((tokens_unfused[live] == np.argmax(score, axis=1)[live]).all(), "launch_decoder token != first maximum of its emb_score")
    print(f"GEMM {fig.label} | rows left to the tie check: {weak} of {c.B}")
    fig.require(weak <= 0.01 * c.B, f"{weak} of {c.B} rows are near-ties: choose another seed")
    return weak


# ---- a tiled GEMM restated in numpy (what the mutants of tests/test_gemm_model_cpu.py break) ---------------------------
def tiled_gemm(x, w, out, slab=32, mutant=None):
    """out[M, N] <- x @ w by 64 x 64 tiles and k slabs of `slab`, fp32 accumulation; `out` arrives holding what memory held
    (a tile that is not written leaves it).  mutant: drop_last_slab | double_slab | skip_last_col_tile |
    last_row_tile_off_by_one | swap_rows."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    M, K = x.shape
    N = w.shape[1]
    slabs = list(range(0, K, slab))
    for m0 in range(0, M, 64):
        m1 = min(m0 + 64, M)
        for n0 in range(0, N, 64):
            n1 = min(n0 + 64, N)
            if mutant == "skip_last_col_tile" and n1 == N and (N % 64 or N > 64):
                continue
            acc = np.zeros((m1 - m0, n1 - n0), np.float32)
            for k0 in slabs:
                if mutant == "drop_last_slab" and k0 == slabs[-1] and (K % slab or len(slabs) > 1):
                    continue
                part = x[m0:m1, k0:k0 + slab] @ w[k0:k0 + slab, n0:n1]
                acc += part
                if mutant == "double_slab" and k0 == slabs[len(slabs) // 2]:
                    acc += part
            if mutant == "last_row_tile_off_by_one" and m1 == M and m1 - m0 > 1 and (M % 64 or M > 64):
                out[m0 + 1:m1, n0:n1] = acc[:-1]
            else:
                out[m0:m1, n0:n1] = acc
    if mutant == "swap_rows" and M > 1:
        out[[0, 1]] = out[[1, 0]]
    return out


def store_values(y32, fmt, mutant=None):
    """fp32 results -> stored values.  mutant: toward_zero (truncation instead of nearest) | no_saturation (fp8: beyond the
    range the bare conversion gives the NaN code)."""
    if fmt == "f32":
        return np.asarray(y32, np.float32)
    if mutant == "toward_zero":
        if fmt == "bf16":
            return (np.ascontiguousarray(y32, np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        r = round_to(y32, "fp8").astype(np.float64)
        a = np.abs(np.asarray(y32, np.float64))
        down = np.abs(r) > a            # rounded away from zero: step one code back
        codes = fp8_bits(np.asarray(y32, np.float32))
        codes = np.where(down & ((codes & 0x7f) > 0), codes - 1, codes).astype(np.uint8)
        return fp8_decode(codes).reshape(np.shape(y32))
    out = round_to(y32, fmt)
    if mutant == "no_saturation" and fmt == "fp8":
        out = np.where(np.abs(np.asarray(y32, np.float32)) >= 464.0, np.float32(np.nan), out)
    return out


def restate(c, e, mutant=None):
    """The call of case c restated on the host with tiled_gemm: returns (after, q_after) in judge's form.  Mutants of the
    scatter: empty_row_q | stray_byte | fill_stops_short | fill_writes_token_L | compact_restart (the token index restarts
    at a tile boundary of the flat list); the others go to tiled_gemm / store_values."""
    rows = list(e.rows)
    if mutant == "fill_stops_short":
        last = {b: int(c.L[b]) - 1 for b, _ in rows}
        rows = [(b, s) for b, s in rows if s != last[b]]
    elif mutant == "fill_writes_token_L":
        rows += [(int(b), int(c.L[b])) for b in c.new_idx[:c.n_new] if 0 < c.L[b] < c.S and
                 (c.layout != "paged" or c.table[b, int(c.L[b]) // PAGE] >= 0)]
    elif mutant == "compact_restart":
        first = {}
        for i, (b, s) in enumerate(rows):
            first.setdefault(b, i)
        rows = [(b, s if (i // 64) * 64 <= first[b] else i - (i // 64) * 64) for i, (b, s) in enumerate(rows)]
    x = c.x_rows(rows, e.embed)
    gm = mutant if mutant in ("drop_last_slab", "double_slab", "skip_last_col_tile", "last_row_tile_off_by_one", "swap_rows") else None
    sm = mutant if mutant in ("toward_zero", "no_saturation") else None
    bb, ss = np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows], np.int64)
    after, q_after = {}, None
    if c.layout == "paged":
        pool = c.pool.copy()
        values = decode(pool, c.fmt)
        for n, seg in (("wk", 1), ("wv", 2)):
            if rows:
                off = _slot_offsets(c, rows, seg)
                y = tiled_gemm(x, c.w[n], values[off].astype(np.float32), mutant=gm)
                pool[off] = encode(store_values(y, c.fmt, sm), c.fmt)   # (a NaN encodes as the NaN code)
        if e.embed and rows:
            pool[_slot_offsets(c, rows, 0)] = encode(x, c.fmt)
        if mutant == "stray_byte":
            pool.view(np.uint8)[pool.view(np.uint8).size // 2 + 1] ^= 1
        after["pool"] = pool
    else:
        kt, v = c.kt.copy(), c.v.copy()
        if rows:
            kt[bb, :, ss] = tiled_gemm(x, c.w["wk"], kt[bb, :, ss], mutant=gm)
            v[bb, ss] = tiled_gemm(x, c.w["wv"], v[bb, ss], mutant=gm)
        if mutant == "stray_byte":
            v.view(np.uint8)[5] ^= 1
        after = {"kt": kt, "v": v}
        if e.embed:
            after["inp"] = c.inp.copy()
            if rows:
                after["inp"][bb, ss] = x
    if e.mode == "latest":
        q_after = c.q.copy()
        if rows:
            q_after[bb] = tiled_gemm(x, c.w["wq"], q_after[bb], mutant=gm)
        if mutant == "empty_row_q":
            q_after[int(np.nonzero(c.L == 0)[0][0])] = 0.0
    return after, q_after

