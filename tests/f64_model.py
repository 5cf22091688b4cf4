"""A plain numpy float64 model of what the attention kernels compute from what memory holds, and the error metrics
of the accuracy tests.  Independent of oracle/oracle_cpu.c: the oracle is an fp32 evaluation, and its
distance to this model is what the tests derive their tolerance from.

Layouts are the project's: q [B, D], kt [B, D, S] (any strides: a transposed view of [B, S, D] rows does), v [B, S, D],
lengths [B].  Slots s >= lengths[b] are never read (they may hold NaN); the model's outputs are 0 there.

Every error is PER ROW and normalised by a condition scale of that row, so that one tolerance serves rows of 2 and
of 4095 tokens; a non-finite value on either side is an infinite error; a row of length 0 has error 0 when every
output the contract defines is exactly 0 and infinity otherwise."""
import math

import numpy as np

from helpers import PAGE


def _f64(a):
    return np.asarray(a).astype(np.float64)


def scores(q, kt, lengths, scale=None):
    """x[b, s] = q[b] . K[b, :, s] / sqrt(D) for s < L (float64, sqrt of the exact integer)."""
    B, D = np.shape(q)
    S = kt.shape[2]
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    x = np.zeros((B, S), np.float64)
    for b in range(B):
        L = int(lengths[b])
        if L:
            x[b, :L] = (_f64(q[b]) @ _f64(kt[b, :, :L])) * scale
    return x


def scores_abs(q, kt, lengths):
    """max_s sum_i |q_i k_is| / sqrt(D): the magnitude a score of the row is summed from (its condition scale)."""
    B, D = np.shape(q)
    out = np.zeros(B, np.float64)
    for b in range(B):
        L = int(lengths[b])
        if L:
            out[b] = (np.abs(_f64(q[b])) @ np.abs(_f64(kt[b, :, :L]))).max() / math.sqrt(D)
    return out


def softmax(x, lengths):
    """Max-subtracted softmax over s < L, exact zero tail."""
    p = np.zeros_like(x, dtype=np.float64)
    for b in range(x.shape[0]):
        L = int(lengths[b])
        if L:
            e = np.exp(x[b, :L] - x[b, :L].max())
            p[b, :L] = e / e.sum()
    return p


def attend(p, v, lengths, absolute=False):
    """o[b] = sum_{s < L} p[b, s] v[b, s] (|v| with absolute=True)."""
    B, D = p.shape[0], v.shape[2]
    o = np.zeros((B, D), np.float64)
    for b in range(B):
        L = int(lengths[b])
        if L:
            vb = _f64(v[b, :L])
            o[b] = _f64(p[b, :L]) @ (np.abs(vb) if absolute else vb)
    return o


def attend_abs(p, v, lengths):
    return attend(p, v, lengths, absolute=True)


class Model:
    """Scores, probabilities, attention and their condition scales for one case."""

    def __init__(self, q, kt, v, lengths):
        self.lengths = np.asarray(lengths).astype(np.int64)
        self.x = scores(q, kt, lengths)
        self.x_scale = scores_abs(q, kt, lengths)
        self.p = softmax(self.x, lengths)
        self.o = attend(self.p, v, lengths)
        self.o_scale = attend_abs(self.p, v, lengths).max(axis=1)


def project_latest(inp, lengths, wk, wq, wv):
    """q, k, v of position L - 1 of every non-empty row (float64 [B, Dout] each; zeros for empty rows) and the
    condition scale of the projection, max_j sum_i |x_i w_ij| per row and weight."""
    B = inp.shape[0]
    out = [np.zeros((B, w.shape[1]), np.float64) for w in (wk, wq, wv)]
    scale = [np.zeros(B, np.float64) for _ in range(3)]
    w64 = [_f64(w) for w in (wk, wq, wv)]
    for b in range(B):
        L = int(lengths[b])
        if L:
            x = _f64(inp[b, L - 1])
            for i in range(3):
                out[i][b] = x @ w64[i]
                scale[i][b] = (np.abs(x) @ np.abs(w64[i])).max()
    return out[1], out[0], out[2], scale[1], scale[0], scale[2]


def gather_pages(pool, table, lengths, n_sequence, emb_dim, seg):
    """[B, S, D] copy of segment `seg` (0 = x, 1 = K, 2 = V) of every live slot s < L through the page layout
    (helpers.pool_index); zeros elsewhere.  `pool` holds VALUES (for bf16 / fp8 pages: the rounded values, which
    float64 represents exactly)."""
    B = len(lengths)
    out = np.zeros((B, n_sequence, emb_dim), pool.dtype)
    within = (np.arange(PAGE) * 3 * emb_dim)[:, None] + seg * emb_dim + np.arange(emb_dim)[None, :]   # [16, D]
    for b in range(B):
        L = int(lengths[b])
        if L:
            pages = table[b, :-(-L // PAGE)]
            assert (pages >= 0).all(), b
            rows = pool[(pages[:, None, None] + within[None]).reshape(-1, emb_dim)]
            out[b, :L] = rows[:L]
    return out


# ---- error metrics (per row) ---------------------------------------------------------------------------------------
def _rows(got, want, lengths, scale, empty_rows_are_zero=False):
    got = np.asarray(got)
    B = got.shape[0]
    err = np.zeros(B, np.float64)
    for b in range(B):
        L = int(lengths[b])
        g = got[b].astype(np.float64)
        if L == 0:
            err[b] = np.inf if empty_rows_are_zero and g.any() else 0.0
            continue
        if not (np.isfinite(g).all() and np.isfinite(want[b]).all()):
            err[b] = np.inf
            continue
        err[b] = np.abs(g - want[b]).max() / scale[b]
    return err


def attention_error(o, model):
    """max_d |o[b, d] - o^[b, d]| / max_d sum_s p^[b, s] |v[b, s, d]|; rows of length 0 must be exactly 0."""
    return _rows(o, model.o, model.lengths, model.o_scale, empty_rows_are_zero=True)


def score_error(x, model):
    """max_{s < L} |x[b, s] - x^[b, s]| / max_s (sum_i |q_i k_is| / sqrt(D)); s >= L is not part of the contract
    (launch_qkt leaves it unwritten), so rows of length 0 have error 0."""
    x = np.asarray(x)
    err = np.zeros(x.shape[0], np.float64)
    for b in range(x.shape[0]):
        L = int(model.lengths[b])
        if L:
            g = x[b, :L].astype(np.float64)
            err[b] = np.abs(g - model.x[b, :L]).max() / model.x_scale[b] if np.isfinite(g).all() else np.inf
    return err


def probability_error(p, model):
    """max_{s < L} |p[b, s] - p^[b, s]| / p^[b, s]; the tail s >= L (the whole row for L = 0) must be exactly 0."""
    p = np.asarray(p)
    err = np.zeros(p.shape[0], np.float64)
    for b in range(p.shape[0]):
        L = int(model.lengths[b])
        g = p[b].astype(np.float64)
        if not np.isfinite(g).all() or g[L:].any():
            err[b] = np.inf
        elif L:
            err[b] = (np.abs(g[:L] - model.p[b, :L]) / model.p[b, :L]).max()
    return err


def projection_error(got, want, lengths, scale):
    """max_j |y[b, j] - y^[b, j]| / max_j sum_i |x_i w_ij| for the rows with L >= 1 (empty rows are left untouched by
    the projection: not compared here)."""
    return _rows(got, want, lengths, scale)


def tolerance(e_oracle):
    """eight times the fp32 oracle's own worst error on the same inputs under the same metric (margin for
    another summation order of the same length), floored at 16 units of 2^-24 for cases where the oracle happens to
    be exact.  Never derived from a kernel."""
    e = float(np.max(e_oracle)) if np.size(e_oracle) else 0.0
    assert np.isfinite(e), "the oracle itself is non-finite on this case"
    return max(8.0 * e, 16.0 * 2.0 ** -24)
