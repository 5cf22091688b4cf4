"""The float64 model of the per-token log-probabilities and top-n alternatives, and the error metric of the
tests that hold the kernels and the engines to it.

For one row of logits x[0..V) the candidates are the finite x, as in the sampler (sampling_ref.kept_set):

    m = max_cand x          lse = m + log(sum_cand exp(x_v - m))          logprob(v) = (x_v - m) - log(sum ...)

natural logarithms of the RAW model distribution: no temperature, top-k or top-p.  The alternatives are the n_top candidates
of largest logit ordered by (logit descending, index ascending); with fewer candidates the rest is id -1, logprob -inf.  A row
that emits no token (length 0, or token -1) reports -inf and padding only.  A chosen token whose own logit is -inf reports
-inf, one whose logit is +inf or NaN reports NaN.

`restate32` says the same in float32 the plain way (max-subtract, one sequential sum, one log).  It is never compared with a
kernel: its own distance to the float64 model on a test's logits is what f64_model.tolerance turns into that test's bound.

TEST INFRASTRUCTURE, like f64_model.py and replay_model.py: never used by the product."""
import numpy as np

import f64_model as fm

MAX_TOP = 8


def row_logprobs(x, dtype=np.float64):
    """logprob of every entry of one row: finite entries as above, -inf entries -inf, +inf and NaN entries NaN.  dtype
    float32 is the restatement: every operation rounded to float32, the sum taken in index order."""
    x = np.asarray(x, np.float32)
    cand = np.isfinite(x)
    out = np.where(np.isneginf(x), -np.inf, np.nan).astype(dtype)
    if not cand.any():
        return out
    xc = x[cand].astype(dtype)
    m = xc.max()
    d = (xc - m).astype(dtype)
    with np.errstate(under="ignore"):
        s = np.cumsum(np.exp(d).astype(dtype), dtype=dtype)[-1]
    out[cand] = (d - np.log(s).astype(dtype)).astype(dtype)
    return out


def row_top(x, n_top):
    """ids of the n_top candidates of largest logit, (logit descending, index ascending); -1 where there are fewer"""
    x = np.asarray(x, np.float32)
    cand = np.nonzero(np.isfinite(x))[0]
    order = cand[np.lexsort((cand, -x[cand].astype(np.float64)))][:n_top]
    return np.concatenate([order, np.full(n_top - len(order), -1)]).astype(np.int64)


def reference(logits, tokens, n_top, dtype=np.float64):
    """(token_logprob [B], top_ids [B, n_top], top_logprobs [B, n_top]) for the tokens a head emitted on these logits;
    a negative token (empty row, no candidate) is a row that emitted nothing."""
    logits = np.asarray(logits, np.float32)
    B = logits.shape[0]
    tok_lp = np.full(B, -np.inf, dtype)
    ids = np.full((B, n_top), -1, np.int64)
    lps = np.full((B, n_top), -np.inf, dtype)
    for b in range(B):
        t = int(tokens[b])
        if t < 0:
            continue
        lp = row_logprobs(logits[b], dtype)
        tok_lp[b] = lp[t]
        ids[b] = row_top(logits[b], n_top)
        lps[b] = np.where(ids[b] >= 0, lp[np.maximum(ids[b], 0)], -np.inf)
    return tok_lp, ids, lps


def restate32(logits):
    """[B, V] float32 restatement of every entry's logprob (as float64 values)"""
    return np.stack([row_logprobs(r, np.float32).astype(np.float64) for r in np.asarray(logits, np.float32)])


def restatement_error(logits):
    """per row: the largest |restatement - model| over the row's candidates, in log units (0 for a row without one)"""
    logits = np.asarray(logits, np.float32)
    e = np.zeros(logits.shape[0])
    for b, r in enumerate(logits):
        cand = np.isfinite(r)
        if cand.any():
            e[b] = np.abs(row_logprobs(r, np.float32).astype(np.float64)[cand] - row_logprobs(r)[cand]).max()
    return e


def tolerance(logits):
    """the bound of a comparison on these logits: f64_model.tolerance of the restatement's own error (never a kernel's)"""
    return fm.tolerance(restatement_error(logits))


def _same(a, b):
    """equal as reported values: both NaN, or the same infinity, or finite (compared by the caller)"""
    return (np.isnan(a) & np.isnan(b)) | ((a == b) & ~np.isfinite(a))


def value_error(got, want):
    """max |got - want| over the entries where the model is finite; infinite where a non-finite entry is not reproduced as
    such (NaN for NaN, the same infinity for an infinity) or where `got` is not finite beside a finite model value"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if got.shape != want.shape:
        return np.inf
    fin = np.isfinite(want)
    if not _same(got[~fin], want[~fin]).all() or not np.isfinite(got[fin]).all():
        return np.inf
    return float(np.abs(got[fin] - want[fin]).max()) if fin.any() else 0.0


def compare(got, logits, tokens, n_top):
    """got = (token_logprob, top_ids, top_logprobs) as a head reported them for `tokens` on `logits`.  Returns (error,
    tolerance, complaints): error = the worst distance of a reported logprob to the model, infinite when the ids are not
    exactly the model's, a padded or no-token entry is not as specified, or the token's logprob is not bit-equal to its entry
    in the list."""
    tok_lp, ids, lps = (np.asarray(a) for a in got)
    w_lp, w_ids, w_lps = reference(logits, tokens, n_top)
    bad = []
    err = max(value_error(tok_lp, w_lp), value_error(lps.reshape(w_lps.shape), w_lps) if n_top else 0.0)
    if n_top and not (ids.reshape(w_ids.shape) == w_ids).all():
        rows = np.nonzero((ids.reshape(w_ids.shape) != w_ids).any(axis=1))[0]
        bad.append(f"top_ids differ from the model's in rows {rows.tolist()}")
        err = np.inf
    if n_top and not bad:
        for b in range(len(w_lp)):
            hit = np.nonzero(w_ids[b] == int(tokens[b]))[0] if int(tokens[b]) >= 0 else []
            if len(hit) and np.float32(tok_lp[b]).tobytes() != np.float32(lps.reshape(w_lps.shape)[b, hit[0]]).tobytes():
                bad.append(f"row {b}: the token's logprob is not bit-equal to its entry in the list")
                err = np.inf
    if not np.isfinite(err) and not bad:
        bad.append("a non-finite, padded or no-token entry is not as specified")
    return err, tolerance(logits), bad


# ---- the score families of the kernel tests (shared by the CPU check that the comparison bites) ---------------------------------
def families(V, seed=0):
    """(logits [8, V] float32, lengths [8]): flat, peaked, +-200 offsets, exact ties inside the top 8, -inf / +inf / NaN
    entries, all -inf, an empty row (length 0), and a plain normal row."""
    rng = np.random.default_rng(seed + V)
    x = np.empty((8, V), np.float32)
    x[0] = 0.25                                                          # flat: every logprob is -log V
    x[1] = rng.standard_normal(V) * 0.1
    x[1, (3 * V) // 7] = 30.0                                            # peaked
    x[2] = rng.standard_normal(V) + np.where(np.arange(V) % 2, 200.0, -200.0)    # exp() of either half alone overflows / vanishes
    x[3] = np.round(rng.standard_normal(V) * 2.0) * 0.5                  # few distinct values: ties everywhere
    x[3, [V - 1, 0, V // 2]] = 9.0                                       # three equal leaders, listed by index
    x[3, [1, V - 2]] = 8.5
    x[4] = rng.standard_normal(V) * 3.0
    x[4, V // 3] = -np.inf
    x[4, V // 2] = np.inf
    x[4, V - 1] = np.nan
    x[5] = -np.inf
    x[6] = rng.standard_normal(V)                                        # never read: the row is empty
    x[7] = rng.standard_normal(V) * 4.0
    lengths = np.array([5, 1, 17, 33, 2, 9, 0, 127], np.int32)
    return x, lengths
