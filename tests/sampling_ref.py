"""numpy reference of the sampled decoder head's contract (include/mli_kernels.h mli_sample_tokens).

Philox4x32-10 vectorised over arrays of counters; the filters in float64 with explicit sorting; the Gumbel noise and the
perturbed scores in float32, operation for operation as the contract states them.  sample_row() also reports how
well-posed its decision is, so that a test can tell a real mismatch from an fp32 rounding tie.
"""
import numpy as np

FLT_MAX = np.float32(3.4028234663852886e38)
M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays (broadcast); returns four uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in (c0, c1, c2, c3)]
    k0 = np.asarray(k0, dtype=np.uint64) & _MASK
    k1 = np.asarray(k1, dtype=np.uint64) & _MASK
    for r in range(10):
        if r:
            k0 = (k0 + W0) & _MASK
            k1 = (k1 + W1) & _MASK
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _MASK]
    return [x.astype(np.uint32) for x in c]


def gumbel(seed, L, V):
    """g(seed, L, v) for v < V, float32."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    v = np.arange(V, dtype=np.int64)
    out = philox4x32_10(v >> 2, np.full(V, L), 0, 0, seed & _MASK, seed >> 32)
    w = np.choose(v & 3, out).astype(np.uint32)
    with np.errstate(divide="ignore"):
        u = ((w >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)  # exact, in (0, 1)
        return (-np.log(-np.log(u))).astype(np.float32)


def greedy(x):
    """The greedy heads' rule: larger value, then lower index, only values above -FLT_MAX; -1 when none."""
    x = np.asarray(x, np.float32)
    ok = x > -FLT_MAX
    if not ok.any():
        return -1
    m = x[ok].max()
    return int(np.nonzero(ok & (x == m))[0][0])


def kept_set(x, T, K, P):
    """Boolean mask of the kept set and the top-p margin (distance of the decisive cumulative masses from P; inf when
    top-p does not apply).  Device out-of-domain rules: K < 0 = 0, P > 1 or NaN = 1."""
    x = np.asarray(x, np.float32)
    cand = np.isfinite(x)
    n = int(cand.sum())
    keep = cand.copy()
    if n == 0:
        return keep, np.inf
    K = max(int(K), 0)
    if 0 < K < n:
        t_k = np.sort(x[cand])[::-1][K - 1]
        keep &= x >= t_k
    margin = np.inf
    if P < 1:  # NaN compares false
        z = (x / np.float32(T)).astype(np.float32).astype(np.float64)
        zk = z[keep]
        q = np.exp(zk - zk.max())
        q /= q.sum()
        xk = x[keep]
        vals, inv = np.unique(xk, return_inverse=True)  # distinct kept values, ascending
        mass = np.cumsum(np.bincount(inv.ravel(), weights=q)[::-1])  # mass of x >= vals[::-1][i]
        vals = vals[::-1]
        hit = np.nonzero(mass >= P)[0]
        i = int(hit[0]) if len(hit) else len(vals) - 1
        t_p = vals[i]
        margin = abs(mass[i] - P) if P > 0 else np.inf
        if i > 0:
            margin = min(margin, abs(mass[i - 1] - P))
        keep &= x >= t_p
    return keep, margin


def sample_row(x, T, K, P, seed, L):
    """(token, gap, margin): gap = best minus second-best perturbed score over the kept set (inf with one element)."""
    x = np.asarray(x, np.float32)
    if L == 0:
        return -1, np.inf, np.inf
    if not T > 0:
        return greedy(x), np.inf, np.inf
    keep, margin = kept_set(x, T, K, P)
    if not keep.any():
        return -1, np.inf, np.inf
    s = ((x / np.float32(T)).astype(np.float32) + gumbel(seed, L, len(x))).astype(np.float32)
    s = np.where(keep, s, -np.inf).astype(np.float32)
    tok = int(np.argmax(s))                              # first index of the maximum
    top2 = np.sort(s[keep].astype(np.float64))[::-1][:2]
    gap = top2[0] - top2[1] if len(top2) > 1 else np.inf
    return tok, gap, margin


def sample(logits, T, K, P, seed, lengths):
    """Row-wise sample_row over [B, V] logits: (tokens, gaps, margins)."""
    out = [sample_row(logits[b], T[b], K[b], P[b], seed[b], lengths[b]) for b in range(logits.shape[0])]
    return (np.array([o[0] for o in out], np.int32), np.array([o[1] for o in out]), np.array([o[2] for o in out]))
