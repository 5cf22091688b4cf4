"""The engine replay audit ("Engine replay audit"): every token an engine emitted, judged on its own against one
causal float64 forward over the item's finished token stream (teacher forcing: the engine's own tokens are the prefix).

Greedy and seeded decoding are per row, so an item's tokens depend only on its own prefix.  For a stream t[0..n) and an
engine description (page element type, n_heads, window, n_sink) the forward is

    x[s] = store(fp32(emb[t_s] + pos[s]))       K = store(x Wk)    V = store(x Wv)    q = x Wq
    scores per head / sqrt(head_dim), mask j <= i and (no window or j > i - W or j < n_sink), softmax, p V per head
    logits[i] = output[i] . emb_table^T         (the logits that choose t[i + 1])

with `store` the identity for fp32 pages and helpers.bf16_round / fp8_round (and bf16-rounded weights) for bf16 / fp8 pages:
what engine_sim.CpuEngine and the heads, window and sinks CPU engines model step by step.

Judges
  greedy       deficit = max(logits[i - 1]) - logits[i - 1][t_i] <= tol for every generated position i
  bookkeeping  prompt intact, the stream ends exactly at the first EOF or at n_sequence tokens, tokens inside [0, V), every
               queued item finished exactly once, stats.total_tokens = the generated tokens (no tolerance)
  sampled      t_i = sampling_ref.sample_row(logits[i - 1], T, K, P, seed, L = i) wherever the draw is well-posed; elsewhere
               t_i lies in the kept set

Tolerances (none fixed in advance, none from a kernel)
  E32        per item, max |fp32 logits - float64 logits| over the audited positions, the fp32 logits from a float32 numpy
             forward over the SAME stored x, K, V (no storage rounding differs)
  tol_logit  f64_model.tolerance(E32 / scale) * scale, scale = the item's largest |logit|: 8 E32, floored at 16 * 2^-24 scale
  tol        2 tol_logit: an argmax over logits each within tol_logit of the model falls short of the maximum by at most that
  E_flip     (native bf16 MFMA, fp8 pages) a K / V element whose exact value lies within emb_dim 2^-24 sum|x_i||w_ij| of the
             midpoint between its two neighbouring stored values may round either way; the logits are re-evaluated under R
             random assignments of those elements (probability 1/2 each) and E_flip is the largest deviation from the
             all-nearest assignment.  tol = 2 (tol_logit + E_flip); E_flip is reported at R / 2 and at R.
  draws      well-posed when the gap of the two best perturbed scores, the top-p margin and the top-k cut all exceed their
             thresholds: 8 x the float32 forward's own error in the perturbed score / in the decisive cumulative mass
             (f64_model.tolerance again), 2 tol_logit for the top-k cut.  At most MASK_CAP of a run's draws may be masked.

MLI_REPLAY_REPORT=<file> writes the figures of every audited case as JSON when the process ends.

TEST INFRASTRUCTURE, like f64_model.py and gemm_model.py: never used by the product."""
import atexit
import hashlib
import json
import math
import os
from dataclasses import asdict, dataclass, field

import numpy as np

import f64_model as fm
import sampling_ref as sr
from helpers import bf16_bits, bf16_round, fp8_bits, fp8_decode, fp8_round

EOF = 1023
FLIP_ROUNDS = 16
MASK_CAP = 0.05
MARGIN = 4.0        # a wrong engine must miss by 4 tol (test_the_comparison_sees_a_scan_that_stops_one_token_early)
U = 2.0 ** -24


@dataclass(frozen=True)
class Spec:
    """What the engine computes: store = "f32" | "bf16" | "fp8" (page element type), heads, window (None = none), sinks;
    flips = the stored K / V bits may differ from the CPU's at rounding boundaries (native bf16 MFMA, fp8 pages)."""
    store: str = "f32"
    n_heads: int = 1
    window: int = None
    n_sink: int = 0
    flips: bool = False

    def name(self):
        return (f"{self.store}{'~' if self.flips else ''} H{self.n_heads} W{self.window or '-'} K{self.n_sink}")


def spec_of_kind(kind_name, n_heads=1, window=None, n_sink=0, native=True):
    """The Spec of an engine kind; `native` = bf16_native_mfma is 1 (PAGED_BF16 only: 0 makes its stored bits the CPU's)."""
    store = {"PAGED_BF16": "bf16", "PAGED_FP8": "fp8"}.get(kind_name, "f32")
    return Spec(store, n_heads, window, n_sink or 0, flips=store == "fp8" or (store == "bf16" and native))


# ---- storage ---------------------------------------------------------------------------------------------------------------
def _round(a32, store):
    return a32 if store == "f32" else (bf16_round(a32) if store == "bf16" else fp8_round(a32))


def weights(model, store):
    """float64 weights as the engine holds them: bf16-rounded beside bf16 / fp8 pages."""
    r = (lambda w: w) if store == "f32" else bf16_round
    return {k: r(np.asarray(model[k], np.float32)).astype(np.float64) for k in ("wk", "wq", "wv")}


def embed(model, tokens, store, first=0, pos_shift=0):
    """x[s] = store(fp32(emb[t_s] + pos[s])) for s = first .. first + len(tokens), float64"""
    t = np.asarray(tokens, np.int64)
    s = np.arange(first, first + len(t)) + pos_shift
    x = np.asarray(model["emb_table"], np.float32)[t] + np.asarray(model["pos_table"], np.float32)[s]
    return _round(x.astype(np.float32), store).astype(np.float64)


def store_neighbours(v, store):
    """(nearest stored value, the other neighbour) of the float64 values v; equal where there is no other (saturation)."""
    f = v.astype(np.float32)
    if store == "bf16":
        bits = bf16_bits(f).reshape(v.shape)
        decode = lambda b: (b.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
        top, sign_bit = 0x7F7F, 0x8000
    else:
        bits = fp8_bits(f).reshape(v.shape)
        decode = lambda b: fp8_decode(b).astype(np.float64)
        top, sign_bit = 126, 0x80
    near = decode(bits)
    mag = (bits & (sign_bit - 1)).astype(np.int64)
    up = np.abs(near) <= np.abs(v)
    other_mag = np.clip(np.where(up | (mag == 0), mag + 1, mag - 1), 0, top)
    other = decode((other_mag | (bits & sign_bit)).astype(bits.dtype))
    return near, other


def project(x, w, store, emb_dim):
    """(stored K or V, the other neighbour, ambiguous) of x w.  fp32 pages: the float64 value itself, nothing ambiguous."""
    v = x @ w
    if store == "f32":
        return v, v, np.zeros(v.shape, bool)
    near, other = store_neighbours(v, store)
    bound = emb_dim * U * (np.abs(x) @ np.abs(w))          # gemm_model's fp32 accumulation ceiling
    amb = (np.abs(v - 0.5 * (near + other)) <= bound) & (other != near)
    return near, other, amb


# ---- the forward -------------------------------------------------------------------------------------------------------------
def causal_mask(n, window=None, n_sink=0):
    i = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    m = j <= i
    if window is not None:
        m &= (j > i - int(window)) | (j < int(n_sink))
    return m


def logits_from_state(x, K, V, wq, emb, mask, n_heads, dtype=np.float64, rows=None):
    """logits [rows, V] from the stored state, every operation in `dtype`.  rows = the positions wanted (default all)."""
    x, K, V, wq, emb = (np.asarray(a).astype(dtype) for a in (x, K, V, wq, emb))
    if rows is not None:
        x, mask = x[rows], mask[rows]
    D = x.shape[1]
    hd = D // n_heads
    q = x @ wq
    out = np.empty((x.shape[0], D), dtype)
    scale = dtype(1.0 / math.sqrt(hd))
    for h in range(n_heads):
        sl = slice(h * hd, (h + 1) * hd)
        s = np.where(mask, (q[:, sl] @ K[:, sl].T) * scale, dtype(-np.inf))
        p = np.exp(s - s.max(axis=1, keepdims=True))
        p = p / p.sum(axis=1, keepdims=True, dtype=dtype)
        out[:, sl] = p @ V[:, sl]
    return out @ emb.T


class Replay:
    """The float64 pass over one token stream: stored state, its rounding ambiguities, and the logits of `rows`."""

    def __init__(self, model, tokens, spec, rows=None):
        n, D = len(tokens), np.shape(model["wk"])[0]
        w = weights(model, spec.store)
        self.spec, self.wq = spec, w["wq"]
        self.emb = np.asarray(model["emb_table"], np.float32).astype(np.float64)
        self.x = embed(model, tokens, spec.store)
        self.K, self.K_other, self.K_amb = project(self.x, w["wk"], spec.store, D)
        self.V, self.V_other, self.V_amb = project(self.x, w["wv"], spec.store, D)
        self.mask = causal_mask(n, spec.window, spec.n_sink)
        self.rows = np.arange(n) if rows is None else np.asarray(rows)
        self.logits = self._logits(self.K, self.V)

    def _logits(self, K, V, dtype=np.float64):
        return logits_from_state(self.x, K, V, self.wq, self.emb, self.mask, self.spec.n_heads, dtype, self.rows)

    def logits32(self):
        """the float32 numpy forward over the same stored state"""
        return self._logits(self.K, self.V, np.float32).astype(np.float64)

    def flip_envelope(self, rounds, seed):
        """(E_flip after rounds / 2 assignments, after all of them, ambiguous elements)"""
        n_amb = int(self.K_amb.sum() + self.V_amb.sum())
        if n_amb == 0 or len(self.rows) == 0:
            return 0.0, 0.0, n_amb
        rng = np.random.default_rng(seed)
        worst, half = 0.0, 0.0
        for r in range(rounds):
            K = np.where(self.K_amb & (rng.random(self.K.shape) < 0.5), self.K_other, self.K)
            V = np.where(self.V_amb & (rng.random(self.V.shape) < 0.5), self.V_other, self.V)
            worst = max(worst, float(np.abs(self._logits(K, V) - self.logits).max()))
            if r + 1 == rounds // 2:
                half = worst
        return half, worst, n_amb


# ---- the judges ----------------------------------------------------------------------------------------------------------------
@dataclass
class Figures:
    what: str = ""
    items: int = 0
    tokens: int = 0
    nonzero_deficits: int = 0
    worst_deficit: float = 0.0
    tol: float = 0.0                 # of the item with the worst deficit / tol (no deficit anywhere: the smallest of any item)
    worst_ratio: float = 0.0         # max over items of worst deficit / tol
    e32: float = 0.0
    e_flip_half: float = 0.0
    e_flip: float = 0.0
    ambiguous: int = 0
    draws: int = 0
    masked_draws: int = 0
    failures: list = field(default_factory=list)
    bookkeeping: list = field(default_factory=list)

    def masked_share(self):
        return self.masked_draws / self.draws if self.draws else 0.0

    def line(self):
        s = (f"REPLAY {self.what}: items {self.items} tokens {self.tokens} non-zero deficits {self.nonzero_deficits} worst "
             f"deficit {self.worst_deficit:.3e} / tol {self.tol:.3e} (worst ratio {self.worst_ratio:.3g}) E32 {self.e32:.3e} "
             f"E_flip {self.e_flip_half:.3e} -> {self.e_flip:.3e} ({self.ambiguous} ambiguous)")
        if self.draws:
            s += f" draws {self.draws} masked {self.masked_draws} ({100 * self.masked_share():.2f} %)"
        return s

    def assert_ok(self):
        assert not self.bookkeeping, f"{self.what}: bookkeeping: " + "; ".join(self.bookkeeping[:5])
        assert not self.failures, f"{self.what}: {len(self.failures)} token(s) rejected: " + "; ".join(self.failures[:5])
        assert self.masked_share() <= MASK_CAP, f"{self.what}: {self.masked_draws} of {self.draws} draws masked"


REPORT = {}


@atexit.register
def _write_report():
    path = os.environ.get("MLI_REPLAY_REPORT")
    if path and REPORT:
        with open(path, "w") as f:
            json.dump(REPORT, f, indent=1)


def bookkeeping(items, finished, n_sequence, n_vocab, total_tokens=None):
    """The list of violations (empty = passes).  items: [(id, prompt)]; finished: [(id, tokens)] as the engine lists them."""
    bad = []
    prompts = {int(i): np.asarray(t) for i, t in items}
    seen = {}
    for item_id, toks in finished:
        item_id, toks = int(item_id), np.asarray(toks)
        if item_id in seen:
            bad.append(f"item {item_id} finished twice")
            continue
        seen[item_id] = toks
        if item_id not in prompts:
            bad.append(f"item {item_id} was never queued")
            continue
        p = prompts[item_id]
        if len(toks) <= len(p) or (toks[:len(p)] != p).any():
            bad.append(f"item {item_id}: prompt not intact")
            continue
        if ((toks < 0) | (toks >= n_vocab)).any():
            bad.append(f"item {item_id}: token outside [0, {n_vocab})")
        gen = toks[len(p):]
        eof = np.nonzero(gen == EOF)[0]
        want = min(len(p) + int(eof[0]) + 1 if len(eof) else n_sequence, n_sequence)
        if len(toks) != want:
            bad.append(f"item {item_id}: {len(toks)} tokens, the stream ends at {want}")
    for item_id in prompts:
        if item_id not in seen:
            bad.append(f"item {item_id} missing")
    if total_tokens is not None:
        gen = sum(len(t) - len(prompts[i]) for i, t in seen.items() if i in prompts)
        if gen != int(total_tokens):
            bad.append(f"total_tokens {int(total_tokens)} but {gen} tokens were generated")
    return bad


def _scaled_tolerance(err, scale):
    scale = max(float(scale), 1e-300)
    return fm.tolerance(err / scale) * scale


def _cum_mass(x, T32, keep, f32):
    """(kept elements by descending x, cumulative softmax mass of x / T over them); float64 sums.  f32 = the division rounded
    to float32 as the contract states it."""
    z = (x.astype(np.float32) / T32).astype(np.float64) if f32 else x / float(T32)
    order = np.argsort(-x, kind="stable")
    order = order[keep[order]]
    q = np.exp(z[order] - z[order].max())
    return order, np.cumsum(q / q.sum())


def _draw(x64, x32, T, K, P, seed, L):
    """One draw judged by the float64 model: dict with the reference's token, the gap of the two best perturbed scores, the
    top-p margin, the top-k cut margin, the float32 forward's error in the perturbed score and in the decisive cumulative
    mass, and the lenient kept-set floor (the logit down to which a masked draw's token is still accepted)."""
    T32 = np.float32(T)
    V = len(x64)
    tok, _, _ = sr.sample_row(x64.astype(np.float32), T, K, P, seed, L)
    g = sr.gumbel(seed, L, V).astype(np.float64)
    order = np.argsort(-x64, kind="stable")
    keep = np.ones(V, bool)
    k_margin, floor = np.inf, -np.inf
    if 0 < K < V:
        keep = x64 >= x64[order[K - 1]]
        k_margin = float(x64[order[K - 1]] - x64[order[K]])
        floor = float(x64[order[K]])                             # one value more than the model keeps
    keep32 = np.ones(V, bool)
    if 0 < K < V:
        keep32 = x32 >= np.sort(x32)[::-1][K - 1]
    margin, e_mass = np.inf, 0.0
    if P < 1:
        kept_sorted, cum64 = _cum_mass(x64, T32, keep, False)
        _, cum32 = _cum_mass(x32, T32, keep32, True)
        hit = np.nonzero(cum64 >= P)[0]
        n = int(hit[0]) if len(hit) else len(kept_sorted) - 1
        ranks = [n] + ([n - 1] if n > 0 else [])
        margin = min(abs(float(cum64[r]) - P) for r in ranks)
        # the float32 forward's cumulative mass at the same RANK (in its own order): continuous under a swap of near-equal logits
        e_mass = max(abs(float(cum64[r] - cum32[min(r, len(cum32) - 1)])) for r in ranks)
        keep = keep & (x64 >= x64[kept_sorted[n]])
        below = kept_sorted[n + 1] if n + 1 < len(kept_sorted) else kept_sorted[n]
        floor = min(floor, float(x64[below])) if n + 1 == len(kept_sorted) else float(x64[below])
    s64 = np.where(keep, x64 / float(T32) + g, -np.inf)
    s32 = ((x32.astype(np.float32) / T32).astype(np.float32) + g.astype(np.float32)).astype(np.float64)
    top2 = np.sort(s64[keep])[::-1][:2]
    gap = float(top2[0] - top2[1]) if len(top2) > 1 else np.inf
    e_score = float(np.abs(s32 - (x64 / float(T32) + g))[keep].max())
    return {"tok": tok, "gap": gap, "margin": margin, "k_margin": k_margin, "e_score": e_score, "e_mass": e_mass,
            "floor": floor, "score_scale": float(np.abs(s64[keep]).max())}


_cache = {}


def _fingerprint(model):
    h = hashlib.sha1()
    for k in ("emb_table", "pos_table", "wk", "wq", "wv"):
        h.update(np.ascontiguousarray(model[k], np.float32).tobytes())
    return h.hexdigest()


def judge_item(model, prompt_len, tokens, spec, params=None, rounds=FLIP_ROUNDS, key=None):
    """One item's figures: dict(deficits, tol, e32, e_flip_half, e_flip, ambiguous, draws, masked, failures).  `params` =
    (temperature, top_k, top_p, seed) of a sampled item.  A sampled item of a kind with rounding flips gets no token judge."""
    tokens = np.asarray(tokens, np.int32)
    ck = (key or _fingerprint(model), spec, params, rounds, int(prompt_len), tokens.tobytes())
    if ck in _cache:
        return _cache[ck]
    n, p = len(tokens), int(prompt_len)
    out = {"deficits": np.zeros(0), "tol": 0.0, "e32": 0.0, "e_flip_half": 0.0, "e_flip": 0.0, "ambiguous": 0, "draws": 0,
           "masked": 0, "failures": [], "tokens": max(n - p, 0)}
    sampled = params is not None and params[0] > 0
    if n > p >= 1 and not (sampled and spec.flips):
        rep = Replay(model, tokens, spec, rows=np.arange(p - 1, n - 1))
        lg = rep.logits                                            # lg[r] chooses tokens[p + r]
        l32 = rep.logits32()
        scale = float(np.abs(lg).max())
        out["e32"] = float(np.abs(l32 - lg).max())
        tol_logit = _scaled_tolerance(out["e32"], scale)
        if spec.flips:
            out["e_flip_half"], out["e_flip"], out["ambiguous"] = rep.flip_envelope(rounds, seed=n * 1000003 + p)
        out["tol"] = 2.0 * (tol_logit + out["e_flip"])
        chosen = tokens[p:]
        if not sampled:
            out["deficits"] = lg.max(axis=1) - lg[np.arange(n - p), chosen]
            for r in np.nonzero(out["deficits"] > out["tol"])[0]:
                out["failures"].append(f"position {p + r}: token {chosen[r]} falls short of the maximum logit by "
                                       f"{out['deficits'][r]:.3e} > tol {out['tol']:.3e}")
        else:
            T, K, P, seed = params
            draws = [_draw(lg[r], l32[r], T, K, P, seed, p + r) for r in range(n - p)]
            thr_gap = _scaled_tolerance(max(d["e_score"] for d in draws), max(d["score_scale"] for d in draws))
            thr_mass = _scaled_tolerance(max(d["e_mass"] for d in draws), 1.0)
            out["draws"] = len(draws)
            out["thr_gap"], out["thr_mass"] = thr_gap, thr_mass
            for r, d in enumerate(draws):
                if d["gap"] > thr_gap and d["margin"] > thr_mass and d["k_margin"] > 2 * tol_logit:
                    if chosen[r] != d["tok"]:
                        out["failures"].append(f"position {p + r}: drew {chosen[r]}, the reference draws {d['tok']} (gap "
                                               f"{d['gap']:.3e}, margin {d['margin']:.3e})")
                else:
                    out["masked"] += 1
                    if not lg[r][chosen[r]] >= d["floor"] - 2 * tol_logit:
                        out["failures"].append(f"position {p + r}: masked draw {chosen[r]} lies outside the kept set")
    if len(_cache) > 4096:
        _cache.clear()
    _cache[ck] = out
    return out


def audit(model, items, finished, spec, n_sequence, total_tokens=None, sampling=None, what="", rounds=FLIP_ROUNDS,
          report=print):
    """Audit one engine run.  items: [(id, prompt)] as queued; finished: [(id, tokens)] (or a dict); sampling: {id:
    (temperature, top_k, top_p, seed)} for the sampled items.  Returns Figures (already reported); Figures.assert_ok() is
    the assertion."""
    if isinstance(finished, dict):
        finished = list(finished.items())
    sampling = sampling or {}
    n_vocab = np.shape(model["emb_table"])[0]
    fig = Figures(what=f"{what} [{spec.name()}]")
    fig.bookkeeping = bookkeeping(items, finished, n_sequence, n_vocab, total_tokens)
    prompts = {int(i): np.asarray(t) for i, t in items}
    key = _fingerprint(model)
    done = set()
    smallest_tol = np.inf
    for item_id, toks in finished:
        item_id = int(item_id)
        toks = np.asarray(toks)
        if item_id in done or item_id not in prompts or ((toks < 0) | (toks >= n_vocab)).any():
            continue
        done.add(item_id)
        j = judge_item(model, len(prompts[item_id]), toks, spec, sampling.get(item_id), rounds, key)
        fig.items += 1
        fig.tokens += j["tokens"]
        fig.e32 = max(fig.e32, j["e32"])
        fig.e_flip_half = max(fig.e_flip_half, j["e_flip_half"])
        fig.e_flip = max(fig.e_flip, j["e_flip"])
        fig.ambiguous += j["ambiguous"]
        fig.draws += j["draws"]
        fig.masked_draws += j["masked"]
        if len(j["deficits"]):
            fig.nonzero_deficits += int((j["deficits"] > 0).sum())
            worst = float(j["deficits"].max())
            fig.worst_deficit = max(fig.worst_deficit, worst)
            smallest_tol = min(smallest_tol, j["tol"])
            if worst > 0 and worst / j["tol"] >= fig.worst_ratio:
                fig.worst_ratio, fig.tol = worst / j["tol"], j["tol"]
        fig.failures += [f"item {item_id} {f}" for f in j["failures"]]
    if fig.worst_ratio == 0.0 and np.isfinite(smallest_tol):
        fig.tol = float(smallest_tol)                # nothing fell short: the strictest item's tolerance
    report(fig.line())
    REPORT[fig.what] = {k: v for k, v in asdict(fig).items() if k not in ("failures", "bookkeeping", "what")}
    REPORT[fig.what].update(rejected_tokens=len(fig.failures), bookkeeping_violations=len(fig.bookkeeping),
                            masked_share=fig.masked_share())
    return fig


def first_divergences(model, items, got, want, spec, report=print, what=""):
    """For the items whose tokens differ from `want` (the CPU engine's): the deficit of the engine's token at the first
    differing position, judged by the replay of the engine's own stream.  Returns [(id, position, deficit, tol)]."""
    out = []
    key = _fingerprint(model)
    for item_id, prompt in items:
        a, b = np.asarray(got[item_id]), np.asarray(want[item_id])
        m = min(len(a), len(b))
        diff = np.nonzero(a[:m] != b[:m])[0]
        if len(diff) == 0 and len(a) == len(b):
            continue
        pos = int(diff[0]) if len(diff) else m
        j = judge_item(model, len(prompt), a, spec, None, FLIP_ROUNDS, key)
        r = pos - len(prompt)
        deficit = float(j["deficits"][r]) if 0 <= r < len(j["deficits"]) else float("nan")
        out.append((item_id, pos, deficit, j["tol"]))
    report(f"REPLAY {what}: {len(out)} of {len(items)} items diverge from the CPU engine; deficit at the first divergence: "
           + (", ".join(f"item {i} @ {pos}: {d:.3e} (tol {t:.3e})" for i, pos, d, t in out) or "-"))
    return out


# ---- generators built on the replay forward: right (fault = None) and wrong ------------------------------------------------------
FAULTS = ("newest token unseen at lengths 1 mod 16", "newest token unseen after a re-prefill", "window lower bound one too low",
          "window lower bound one too high", "one sink too many", "one sink too few", "sinks ignored", "heads ignored",
          "scale 1/sqrt(emb_dim)", "position L - 1 for the appended token", "length never advanced",
          "V of the previous token reused")


def generate(model, prompt, spec, n_sequence, fault=None, params=None, item_id=0, draw=None):
    """Decode one item autoregressively on the float64 forward (the token choice on the float32-rounded logits, as the CPU
    engines choose), optionally with one fault injected.  params = (T, K, P, seed) draws with sampling_ref.sample_row; `draw`
    replaces that call (the sampled mutants)."""
    D = np.shape(model["wk"])[0]
    w = weights(model, spec.store)
    emb = np.asarray(model["emb_table"], np.float32).astype(np.float64)
    toks = [int(t) for t in prompt]
    p = len(toks)
    H, W, K = spec.n_heads, spec.window, spec.n_sink
    if fault == "heads ignored":
        H = 1
    if fault == "window lower bound one too low":
        W += 1
    if fault == "window lower bound one too high":
        W -= 1
    if fault == "one sink too many":
        K += 1
    if fault == "one sink too few":
        K -= 1
    if fault == "sinks ignored":
        K = 0
    hd = D // H
    scale = 1.0 / math.sqrt(D if fault == "scale 1/sqrt(emb_dim)" else hd)
    x = np.zeros((n_sequence, D))
    Kc = np.zeros((n_sequence, D))
    Vc = np.zeros((n_sequence, D))
    x[:p] = embed(model, toks, spec.store)
    Kc[:p] = project(x[:p], w["wk"], spec.store, D)[0]
    Vc[:p] = project(x[:p], w["wv"], spec.store, D)[0]
    reprefill_at = p + 3 + 5 * (item_id % 4)           # the simulated preemption: the row is prefilled again at this length
    while True:
        L = len(toks)
        j = np.arange(L)
        m = np.ones(L, bool) if W is None else (j > L - 1 - W) | (j < K)
        if fault == "length never advanced":
            m &= j < p
        unseen = (fault == "newest token unseen at lengths 1 mod 16" and L % 16 == 1) or \
                 (fault == "newest token unseen after a re-prefill" and L == reprefill_at)
        if unseen and m[:L - 1].any():
            m[L - 1] = False
        q = x[L - 1] @ w["wq"]
        out = np.empty(D)
        for h in range(H):
            sl = slice(h * hd, (h + 1) * hd)
            s = np.where(m, (Kc[:L, sl] @ q[sl]) * scale, -np.inf)
            pr = np.exp(s - s.max())
            out[sl] = (pr / pr.sum()) @ Vc[:L, sl]
        logits = (emb @ out).astype(np.float32)
        if params is None:
            tok = sr.greedy(logits)
        else:
            tok = (draw or sr.sample_row)(logits, *params, L)
            tok = tok[0] if isinstance(tok, tuple) else tok
        toks.append(int(tok))
        if len(toks) >= n_sequence or tok == EOF:
            return np.asarray(toks, np.int32)
        x[L] = embed(model, [tok], spec.store, first=L, pos_shift=-1 if fault == "position L - 1 for the appended token" else 0)
        Kc[L] = project(x[L:L + 1], w["wk"], spec.store, D)[0]
        Vc[L] = Vc[L - 1] if fault == "V of the previous token reused" else project(x[L:L + 1], w["wv"], spec.store, D)[0]


# ---- the sampled workload, shared by the CPU check of the masked-draw cap and the GPU engine tests ---------------------------------
SAMPLED_SHAPE = dict(B=8, S=128, D=128, V=1024, W=40)
SAMPLED_PARAMS = {"top-k": (0.8, 40, 1.0), "top-p": (0.8, 0, 0.95)}


def sampled_workload(which):
    """(model, items, {id: (T, K, P, seed)}): 16 items with prompts of 3 .. 60 tokens, the odd ones sampled with their own
    seeds, the even ones greedy.  emb_dim 128 so that 4 heads have head_dim 32."""
    from engine_sim import make_items, make_model
    s = SAMPLED_SHAPE
    model = make_model(9301, s["V"], s["S"], s["D"])
    items = make_items(9302, 16, 3, 60)
    T, K, P = SAMPLED_PARAMS[which]
    return model, items, {i: (T, K, P, 1000003 * i + 17) for i, _ in items if i % 2}
