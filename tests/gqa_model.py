"""Grouped-query attention for the tests: n_kv_heads = Hkv K/V heads serve n_heads = H query heads, query head h
attending K/V head h // g, g = H // Hkv, whose columns are [(h // g) * hd, (h // g + 1) * hd) of K and V; the columns
>= Dkv = Hkv * hd are never read.  That is multi-head attention with H heads on EXPANDED operands, in which the K and V
column block of head h is a copy of block h // g -- so the references are the existing ones (heads_model.oracle_heads /
HeadsModel, or under a window with sinks sinks_model.oracle_sinks / model_sinks) applied to expand_kv(K), expand_kv(V), and
for an engine to a model with expand_kv(Wk), expand_kv(Wv).  Errors and tolerance are heads_model's: per (row, query head),
f64_model.tolerance from the oracle's own error on the heads of the same score family.

Score families are assigned per K/V HEAD (heads_model.families_of over Hkv) and built on the group's first query head
h0 = j * g with accuracy_cases.apply_family on (q[h0], K[j]).  The families that modify K (offset+-, late_peak, early_peak)
do so along q[h0]: the other query heads of the group are q[h0] times distinct positive factors, so their scores carry the
same shift scaled (+-200 f, +30 f with f in [1, 1.875]: still an overflow without the maximum, still a dominating peak)
while every head's softmax differs.  `peaked` scales each head's own random q; `flat` keeps independent random query heads.

TEST INFRASTRUCTURE, like heads_model.py: never used by the product."""
import math

import numpy as np

import f64_model as fm
import heads_model as hm
import sinks_model as sm
from accuracy_cases import apply_family

P = (0, 0)   # (window, n_sink) of the plain form; (W, 0) = window alone; (W, K) = window with sinks

# heads_model.HEAD_SHAPES with (H, Hkv, forms) lists: Hkv = 1 (all), g = 2 (301, 302, 304, 307), 4 (302, 304, 305, 306), 8
# (302), 3 (303: H 3 / Hkv 1 and H 6 / Hkv 2); both page types; one lane load per row (NJ 1: fp32 D <= 256, bf16 D <= 512)
# and two (fp32 D 512, bf16 D 1024)
GQA_SHAPES = [
    (301, 40, 64, 64, ((2, 1, (P, (17, 0), (16, 4))),), ("f32", "bf16"), (64,)),
    (302, 24, 256, 512, ((8, 4, (P,)), (8, 2, ((100, 20),)), (8, 1, ((40, 0),)), (2, 1, (P,))), ("f32", "bf16"), (64, 256)),
    (303, 24, 256, 192, ((3, 1, (P, (100, 4))), (6, 2, (P,))), ("f32", "bf16"), (64, 256)),
    (304, 20, 1024, 256, ((8, 2, ((100, 0), (256, 0))), (2, 1, (P, (513, 4)))), ("f32", "bf16"), (64, 256)),
    (305, 24, 512, 1024, ((8, 2, (P, (130, 4))),), ("bf16",), (64, 256)),
    (306, 16, 4096, 512, ((4, 1, (P, (1024, 0))),), ("bf16",), (64, 1024)),
    (307, 700, 128, 64, ((2, 1, (P, (50, 4))),), ("f32",), (64,)),
]
assert [s[:4] for s in GQA_SHAPES] == [s[:4] for s in hm.HEAD_SHAPES]

FACTORS = tuple(1.0 + 0.125 * i for i in range(8))   # of the group's query heads along its first one (families that modify K)


def expand_kv(a, H, Hkv, axis=-1):
    """The expanded operand: along `axis` (D columns: K^T [B, D, S] axis 1, V [B, S, D] axis 2, a weight [D_in, D] axis 1)
    block h of the result is block h // (H // Hkv) of `a`.  Columns >= Hkv * hd of `a` do not reach the result."""
    a = np.asarray(a)
    D = a.shape[axis]
    assert D % H == 0 and H % Hkv == 0 and 1 <= Hkv <= H
    hd, g = D // H, H // Hkv
    cols = np.concatenate([np.arange((h // g) * hd, (h // g + 1) * hd) for h in range(H)])
    return np.ascontiguousarray(np.take(a, cols, axis=axis))


def expand_model(model, H, Hkv):
    """The engine model (engine_sim.make_model) with expanded Wk / Wv: n_heads heads on it are grouped-query attention on
    `model`, whose Wk / Wv keep their [D, D] shape with only the first Hkv * hd output columns mattering."""
    m = dict(model)
    m["wk"], m["wv"] = expand_kv(model["wk"], H, Hkv, 1), expand_kv(model["wv"], H, Hkv, 1)
    return m


def kv_families(assignment, Hkv):
    return hm.families_of(assignment, Hkv)


def head_families(assignment, H, Hkv):
    """the family of every QUERY head: its K/V head's"""
    fams = kv_families(assignment, Hkv)
    return tuple(fams[h // (H // Hkv)] for h in range(H))


def apply_gqa_families(c, H, Hkv, assignment):
    """(q [B, D], kt [B, D, S]): the assignment's family applied per K/V head on the group's first query head; the K/V head's
    columns are [j * hd, (j + 1) * hd) of kt, the columns >= Hkv * hd stay as generated.  c is not modified."""
    q = c["q_output"].copy()
    kt = c["kt_cache"].copy()
    D = q.shape[1]
    g = H // Hkv
    for j, family in enumerate(kv_families(assignment, Hkv)):
        ksl = hm.head_slice(j, H, D)                     # block j of K: hd columns
        modifies_k = family not in ("flat", "peaked")
        for i in range(g):
            qsl = hm.head_slice(j * g + i, H, D)
            if modifies_k and i > 0:
                q[:, qsl] = np.float32(FACTORS[i]) * q[:, hm.head_slice(j * g, H, D)]
                continue
            sub = {"q_output": np.ascontiguousarray(q[:, qsl]), "kt_cache": np.ascontiguousarray(kt[:, ksl, :]),
                   "lengths": c["lengths"]}
            q[:, qsl], k_new = apply_family(sub, family)
            if i == 0:
                kt[:, ksl, :] = k_new
    return q, kt


def oracle_gqa(oracle, q, kt, v, lengths, H, Hkv, W=0, K=0):
    """attention_result [B, D] of the fp32 CPU oracle on the expanded operands (W 0: no window)"""
    S = kt.shape[2]
    return sm.oracle_sinks(oracle, q, expand_kv(kt, H, Hkv, 1), expand_kv(v, H, Hkv, 2), lengths, H, W if W > 0 else S, K)


def model_gqa(q, kt, v, lengths, H, Hkv, W=0, K=0):
    """heads_model.HeadsModel (float64 per query head) on the expanded operands"""
    S = kt.shape[2]
    return sm.model_sinks(q, expand_kv(kt, H, Hkv, 1), expand_kv(v, H, Hkv, 2), lengths, H, W if W > 0 else S, K)


def compare(o, o_oracle, model, fams, what="", report=print):
    """heads_model.compare with the families of the query heads given (head_families): per score family, the worst (row,
    head) error of `o` against f64_model.tolerance of the oracle's error on the heads of that family."""
    err, e_or = hm.heads_error(o, model), hm.heads_error(o_oracle, model)
    assert len(fams) == model.H
    out = []
    for family in sorted(set(fams)):
        cols = [h for h in range(model.H) if fams[h] == family]
        tol = fm.tolerance(e_or[:, cols])
        worst = float(err[:, cols].max())
        report(f"GQA {what} | {family}: got {worst:.3e}  oracle {float(e_or[:, cols].max()):.3e}  tol {tol:.3e}")
        out.append((family, worst, tol))
    return out


assert_within = hm.assert_within


# ---- wrong models: the faults a grouped-query kernel actually has ------------------------------------------------------------
def _heads_with(q, kt, v, lengths, H, k_block, v_block, scale=None):
    """float64 attention in which query head h reads K block k_block(h) and V block v_block(h)"""
    D = q.shape[1]
    o = np.zeros(q.shape, np.float64)
    for h in range(H):
        ks, vs = hm.head_slice(k_block(h), H, D), hm.head_slice(v_block(h), H, D)
        x = fm.scores(q[:, hm.head_slice(h, H, D)], kt[:, ks, :], lengths, **({} if scale is None else {"scale": scale}))
        o[:, hm.head_slice(h, H, D)] = fm.attend(fm.softmax(x, lengths), v[:, :, vs], lengths)
    return o


def wrong_modulo(q, kt, v, lengths, H, Hkv):
    """K/V head h % Hkv instead of h // g"""
    return _heads_with(q, kt, v, lengths, H, lambda h: h % Hkv, lambda h: h % Hkv)


def wrong_grouping_ignored(q, kt, v, lengths, H, Hkv):
    """head h reads block h"""
    return _heads_with(q, kt, v, lengths, H, lambda h: h, lambda h: h)


def wrong_v_not_grouped(q, kt, v, lengths, H, Hkv):
    g = H // Hkv
    return _heads_with(q, kt, v, lengths, H, lambda h: h // g, lambda h: h)


def wrong_k_not_grouped(q, kt, v, lengths, H, Hkv):
    g = H // Hkv
    return _heads_with(q, kt, v, lengths, H, lambda h: h, lambda h: h // g)


def wrong_scale_dkv(q, kt, v, lengths, H, Hkv):
    """grouped, but divided by sqrt(Dkv)"""
    g = H // Hkv
    return _heads_with(q, kt, v, lengths, H, lambda h: h // g, lambda h: h // g,
                       scale=1.0 / math.sqrt(Hkv * (q.shape[1] // H)))


WRONG_MODELS = {"K/V head h % Hkv": wrong_modulo, "grouping ignored": wrong_grouping_ignored, "K grouped, V not": wrong_v_not_grouped,
                "V grouped, K not": wrong_k_not_grouped, "scale 1/sqrt(Dkv)": wrong_scale_dkv}


def wrong_is_the_right_model(name, H, Hkv):
    """where a wrong model IS grouped-query attention and no input can tell: h % Hkv == h // g for every head exactly when
    Hkv == 1 (both 0); 1 / sqrt(Dkv) is the right scale when Hkv == 1 (Dkv = hd)"""
    return Hkv == 1 and name in ("K/V head h % Hkv", "scale 1/sqrt(Dkv)")
