"""What grouped-query attention saves the lean paged scan: mli_decode_scan_paged_gqa with n_kv_heads < n_heads against the
multi-head scan (n_kv_heads = n_heads, the existing kernels) at the same shape, on the same pages, in the same process.

  config-4 shape  bf16, B = 1024, S = 4096, D = 512: H = 8 with Hkv = 8 (baseline), 4, 2, 1; H = 16 with Hkv = 16 (baseline), 4
  config-3 shape  fp32, B = 256, S = 1024, D = 256: H = 4 with Hkv = 4 (baseline), 2, 1
  each without a window and with a window of 1024 tokens (at the config-3 shape that is n_sequence: no window, the same scan)
  engine          PAGED_BF16, B = 1024, S = 4096, D = 512, H = 8, 2048 items, Hkv = 8 against Hkv = 2, tokens/s

A variant reads the algorithmic bytes sum_rows live(L) * 2 * Dkv * e (live(L) = L, or min(L, W) under a window), 1 / g of
its baseline's; the load instructions are the baseline's.  Reported per variant: us per launch, those bytes, time / baseline
and 1 / g beside it.  HIP events on the launch stream; after a warm-up, five regions of 20 launches per variant, the variants
interleaved region by region; median / min / max of the regions' per-launch time.

  python tools/gqa_probe.py [--out profiles/gqa_probe.json] [--no-engine] [--regions 5] [--launches 20]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from min_llm_inference_amd import engine as eng, load_library, ops  # noqa: E402

WINDOW = 1024


def region(fn, launches, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        fn()
    e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us


def scan_table(name, dtype, pairs, args, dev, side):
    """pairs: (H, Hkv) with the baseline (Hkv == H) of every H among them"""
    wl = bench.Workload(name, dev, 0x5EED, headroom=8, dtype=dtype)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    wl.q_output.copy_(torch.rand(wl.B, wl.D, device=dev, generator=g) * 2 - 1)
    L = np.minimum(np.asarray(wl.lengths_host).astype(np.int64), wl.S)

    def launch(H, Hkv, W):
        return lambda: ops.decode_scan_paged_gqa(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, W, 0,
                                                 wl.elem, wl.S)

    variants = {f"H{H}_Hkv{Hkv}_W{W or '-'}": (H, Hkv, W, launch(H, Hkv, W)) for W in (0, WINDOW) for H, Hkv in pairs}
    ops.workspace_for(wl.B, wl.S, wl.D, dev, max(H for H, _ in pairs))   # grown once, before anything is timed
    times = {k: [] for k in variants}
    for _, _, _, fn in variants.values():
        for _ in range(5):
            fn()
    side.synchronize()
    for _ in range(args.regions):
        for k, (_, _, _, fn) in variants.items():
            times[k].append(region(fn, args.launches, side))
    out = {"shape": {"dtype": dtype, "B": wl.B, "S": wl.S, "D": wl.D}, "regions": args.regions,
           "launches_per_region": args.launches, "variants": {}}
    for k, t in times.items():
        H, Hkv, W, _ = variants[k]
        live = np.minimum(L, W) if W else L
        alg = int(live.sum()) * 2 * (wl.D // H * Hkv) * wl.esize
        med = float(np.median(t))
        base = float(np.median(times[f"H{H}_Hkv{H}_W{W or '-'}"]))
        out["variants"][k] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                              "kv_MB": round(alg / 1e6, 1), "kv_TBps": round(alg / med / 1e6, 3),
                              "time_vs_baseline": round(med / base, 3), "one_over_g": round(Hkv / H, 3)}
    del wl
    torch.cuda.empty_cache()
    return out


def engine_rate(n_heads, n_kv_heads, dev):
    B, S, D, V = 1024, 4096, 512, bench.N_VOCAB
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * B)]
    e = eng.Engine(eng.PAGED_BF16, B, S, D, V, *weights, n_blocks=B * S // 32, device=dev.index, n_heads=n_heads,
                   n_kv_heads=n_kv_heads)
    for i, toks in items:
        e.add_item(i, toks)
    st = e.run()
    e.close()
    assert st.finished == 2 * B
    return {"tokens": int(st.total_tokens), "seconds": round(st.seconds, 3), "iterations": int(st.iterations),
            "tokens_per_s": round(st.total_tokens / st.seconds, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    load_library()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)
    out = {}
    with torch.cuda.stream(side):
        out["config4_bf16"] = scan_table("c4", "bf16", ((8, 8), (8, 4), (8, 2), (8, 1), (16, 16), (16, 4)), args, dev, side)
        out["config3_f32"] = scan_table("c3", "f32", ((4, 4), (4, 2), (4, 1)), args, dev, side)
    if not args.no_engine:
        e = out["engine_paged_bf16_B1024_S4096_D512_H8_2048_items"] = {f"Hkv{k}": engine_rate(8, k, dev) for k in (8, 2)}
        e["Hkv2_vs_Hkv8_tokens_per_s"] = round(e["Hkv2"]["tokens_per_s"] / e["Hkv8"]["tokens_per_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
