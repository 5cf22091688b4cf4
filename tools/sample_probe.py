#!/usr/bin/env python3
"""Cost of the sampled decoder head.  Not bench.py, which measures the greedy product and does not change.

  --part kernels   us per mli_sample_tokens launch (HIP events; run under `rocprofv3 --kernel-trace --stats` for the
                   kernel's own time) at B = 1024, V = 1024 and B = 256, V = 50257, each for T only, T + top-k 50 and
                   T + top-p 0.9
  --part engine    engine tokens/s at the e1 shape (bench.py --mode engine: paged_gemm, pipelined loop, B = 1024, S = 128,
                   D = 2048, V = 1024, 4096 pages, 2048 prompts of U[1, 64] tokens) with every item greedy and with every
                   item at T = 0.8, top-p 0.95
Prints one JSON object.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from min_llm_inference_amd import engine as eng  # noqa: E402
from min_llm_inference_amd import ops  # noqa: E402


def kernels(reps):
    dev = torch.device("cuda:0")
    out = []
    for B, V in ((1024, 1024), (256, 50257)):
        rng = np.random.default_rng(B + V)
        x = torch.from_numpy((rng.standard_normal((B, V)) * 2).astype(np.float32)).to(dev)
        lengths = torch.full((B,), 17, dtype=torch.int32, device=dev)
        seed = torch.arange(B, dtype=torch.int64, device=dev)
        tokens = torch.empty(B, dtype=torch.int32, device=dev)
        for name, K, P in (("T", 0, 1.0), ("T+K50", 50, 1.0), ("T+P0.9", 0, 0.9)):
            T = torch.full((B,), 0.8, device=dev)
            k = torch.full((B,), K, dtype=torch.int32, device=dev)
            p = torch.full((B,), P, device=dev)
            run = lambda: ops.sample_tokens(x, T, k, p, seed, lengths, tokens)  # noqa: E731
            for _ in range(5):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                run()
            e1.record()
            torch.cuda.synchronize()
            out.append({"B": B, "V": V, "params": name, "us_per_launch_events": round(e0.elapsed_time(e1) / reps * 1e3, 2)})
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
    res = {}
    for name, kw in (("greedy", None), ("sampled_T0.8_P0.95", dict(temperature=0.8, top_p=0.95))):
        rates, toks, iters = [], [], []
        for r in range(repeats):
            e = eng.Engine(eng.PAGED_GEMM, B, S, D, V, *weights, n_blocks=B * S // 32)
            for i, t in items:
                e.add_item(i, t, **(dict(kw, seed=i) if kw else {}))
            st = e.run()
            e.close()
            rates.append(st.total_tokens / st.seconds)
            toks.append(st.total_tokens)
            iters.append(st.iterations)
        res[name] = {"tokens_per_s_median": float(np.median(rates)), "all": rates, "tokens": toks, "iterations": iters,
                     "us_per_token_step": [1e6 / r * B for r in rates]}
    res["sampled_over_greedy"] = res["sampled_T0.8_P0.95"]["tokens_per_s_median"] / res["greedy"]["tokens_per_s_median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["kernels", "engine", "all"], default="all")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "time": time.strftime("%Y-%m-%d %H:%M:%S")}
    if a.part in ("kernels", "all"):
        out["kernels"] = kernels(a.reps)
    if a.part in ("engine", "all"):
        out["engine_e1"] = engine(a.repeats)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
