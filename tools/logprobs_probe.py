#!/usr/bin/env python3
"""Cost of the log-probability heads.  Not bench.py, which measures the greedy product and does not change.

  --part kernels   us per launch of the token pick (HIP events around `--reps` launches -- ten times as many at the small
                   shape, so that a region lasts tens of milliseconds --, after a warm-up of every variant) at
                   B = 1024, V = 1024 and B = 256, V = 50257, for T only and T + top-p 0.9, in four columns measured region
                   by region in turn, `--rounds` times (the median and the spread of the rounds are reported):
                     baseline   mli_sample_tokens of another build of the library (--baseline-lib: the parent commit's),
                                omitted without one
                     off        mli_sample_tokens of this build (the same kernel: must sit inside +-3 % of the baseline)
                     n_top 0    mli_sample_tokens_logprobs, the token's logprob alone
                     n_top 8    mli_sample_tokens_logprobs with 8 alternatives
  --part engine    engine tokens/s at the e1 shape (paged_gemm, pipelined loop, B = 1024, S = 128, D = 2048, V = 1024, 4096
                   pages, 2048 prompts of U[1, 64] tokens), median of `--repeats` runs taken in turn: every item greedy
                   (the fused head) against greedy with logprobs (n_top 0 and 8: the sampled head family, materialised
                   logits), and every item at T = 0.8, top-p 0.95 against the same with logprobs
Prints one JSON object.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from min_llm_inference_amd import _lib  # noqa: E402
from min_llm_inference_amd import engine as eng  # noqa: E402
from min_llm_inference_amd import ops  # noqa: E402


def _baseline(path):
    lib = ctypes.CDLL(path)
    lib.mli_sample_tokens.argtypes = _lib.SIGNATURES["mli_sample_tokens"]
    lib.mli_sample_tokens.restype = ctypes.c_int
    return lib


def kernels(reps, rounds, baseline_path):
    dev = torch.device("cuda:0")
    lib = ops.load_library()
    base = _baseline(baseline_path) if baseline_path else None
    out = []
    for B, V, n_launches in ((1024, 1024, 10 * reps), (256, 50257, reps)):
        rng = np.random.default_rng(B + V)
        x = torch.from_numpy((rng.standard_normal((B, V)) * 2).astype(np.float32)).to(dev)
        lengths = torch.full((B,), 17, dtype=torch.int32, device=dev)
        seed = torch.arange(B, dtype=torch.int64, device=dev)
        tokens = torch.empty(B, dtype=torch.int32, device=dev)
        lp = torch.empty(B, dtype=torch.float32, device=dev)
        ids = torch.empty((B, 8), dtype=torch.int32, device=dev)
        tops = torch.empty((B, 8), dtype=torch.float32, device=dev)
        p_ = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        for name, P in (("T", 1.0), ("T+P0.9", 0.9)):
            T = torch.full((B,), 0.8, device=dev)
            k = torch.zeros(B, dtype=torch.int32, device=dev)
            p = torch.full((B,), P, device=dev)
            plain = (p_(x), p_(T), p_(k), p_(p), p_(seed), p_(lengths), p_(tokens))

            def pick(which):
                return lambda: which.mli_sample_tokens(*plain, B, V, None, 0, st)

            def with_logprobs(n_top):
                return lambda: lib.mli_sample_tokens_logprobs(*plain, p_(lp), p_(ids), p_(tops), B, V, n_top, None, 0, st)

            columns = {"off": pick(lib), "n_top_0": with_logprobs(0), "n_top_8": with_logprobs(8)}
            if base is not None:
                columns = {"baseline": pick(base), **columns}
            for run in columns.values():
                for _ in range(5):
                    assert run() == 0
            torch.cuda.synchronize()
            took = {c: [] for c in columns}
            for _ in range(rounds):
                for c, run in columns.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n_launches):
                        run()
                    e1.record()
                    torch.cuda.synchronize()
                    took[c].append(e0.elapsed_time(e1) / n_launches * 1e3)
            row = {"B": B, "V": V, "params": name, "launches_per_region": n_launches, "rounds": rounds}
            for c, v in took.items():
                row[c] = {"us_per_launch_events_median": round(float(np.median(v)), 2), "min": round(min(v), 2),
                          "max": round(max(v), 2)}
            if base is not None:
                row["off_over_baseline"] = round(row["off"]["us_per_launch_events_median"] /
                                                 row["baseline"]["us_per_launch_events_median"], 4)
            out.append(row)
    return out


def engine(repeats):
    B, S, D, V = 1024, 128, 2048, 1024
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * B)]
    sampled = dict(temperature=0.8, top_p=0.95)
    variants = {"greedy": (None, None), "greedy_logprobs_0": (None, 0), "greedy_logprobs_8": (None, 8),
                "sampled_T0.8_P0.95": (sampled, None), "sampled_logprobs_0": (sampled, 0), "sampled_logprobs_8": (sampled, 8)}
    res = {name: {"all": [], "tokens": [], "iterations": []} for name in variants}
    for r in range(repeats):
        for name, (kw, n_top) in variants.items():
            e = eng.Engine(eng.PAGED_GEMM, B, S, D, V, *weights, n_blocks=B * S // 32, logprobs=n_top)
            for i, t in items:
                e.add_item(i, t, **(dict(kw, seed=i) if kw else {}))
            st = e.run()
            e.close()
            res[name]["all"].append(st.total_tokens / st.seconds)
            res[name]["tokens"].append(st.total_tokens)
            res[name]["iterations"].append(st.iterations)
    for v in res.values():
        v["tokens_per_s_median"] = float(np.median(v["all"]))
        v["spread"] = (max(v["all"]) - min(v["all"])) / v["tokens_per_s_median"]
    ratio = lambda a, b: res[a]["tokens_per_s_median"] / res[b]["tokens_per_s_median"]  # noqa: E731
    res["greedy_logprobs_0_over_greedy"] = ratio("greedy_logprobs_0", "greedy")
    res["greedy_logprobs_8_over_greedy"] = ratio("greedy_logprobs_8", "greedy")
    res["sampled_logprobs_0_over_sampled"] = ratio("sampled_logprobs_0", "sampled_T0.8_P0.95")
    res["sampled_logprobs_8_over_sampled"] = ratio("sampled_logprobs_8", "sampled_T0.8_P0.95")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "engine", "all"], default="all")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None, help="libmli_hip.so of the parent commit (the kernels' baseline column)")
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%d %H:%M:%S")}
    if a.part in ("kernels", "all"):
        out["kernels"] = kernels(a.reps, a.rounds, a.baseline_lib)
    if a.part in ("engine", "all"):
        out["engine_e1"] = engine(a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
