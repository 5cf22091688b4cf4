"""The grouped-query scan on matrix instructions (mli_decode_scan_paged_gqa_mfma) timed on an MI355X.

  (a) config-4 shape  bf16, B = 1024, S = 4096, D = 512, H = 8, ragged lengths, Hkv = 4 / 2 / 1 (g = 2 / 4 / 8): the new scan
      against mli_decode_scan_paged_gqa (the lane-group kernel, unchanged) on the same pages, in alternated regions; and both
      against the multi-head scan (Hkv = 8), the baseline the byte ratios 1 / g refer to
  (b) wide shape      bf16, B = 256, S = 4096, 32 heads of 128 on 8 K/V heads (D = 4096), lengths U[S/4, 3S/4]: K/V bytes per
      second of the new scan (no other scan takes the shape) against the 8 TB/s peak and against the streaming-read ceiling
      (mli_stream_read over the same pool, 4 GiB per launch, timed in the same alternated regions)
  (c) end to end      the PAGED_BF16 engine at that shape (n_vocab 1024, prompts U[S/4, 3S/4], every item decoded to n_sequence,
      the pipelined loop): generated tokens per second of wall time of one run, prefill included

HIP events on the launch stream; after a warm-up, --regions regions of --launches launches per variant, interleaved region by
region; median / min / max of the regions' per-launch time.

  python tools/gqa_mfma_probe.py [--out profiles/gqa_mfma_probe.json] [--regions 7] [--launches 20] [--no-wide] [--no-engine]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gqa_probe import region  # noqa: E402
from min_llm_inference_amd import load_library, ops  # noqa: E402


def timed(variants, args, side):
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(5):
            fn()
    side.synchronize()
    for _ in range(args.regions):
        for k, fn in variants.items():
            times[k].append(region(fn, args.launches, side))
    return times


def stats(t, kv_bytes):
    med = float(np.median(t))
    return {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1), "kv_MB": round(kv_bytes / 1e6, 1),
            "kv_TBps": round(kv_bytes / med / 1e6, 3)}


def config4(args, dev, side):
    wl = bench.Workload("c4", dev, 0x5EED, headroom=8, dtype="bf16")
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    wl.q_output.copy_(torch.rand(wl.B, wl.D, device=dev, generator=g) * 2 - 1)
    live = int(np.minimum(np.asarray(wl.lengths_host).astype(np.int64), wl.S).sum())
    H = 8
    ops.workspace_for(wl.B, wl.S, wl.D, dev, H)
    variants = {"lanes_Hkv8": lambda: ops.decode_scan_paged_gqa(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, H, 0,
                                                                 0, wl.elem, wl.S)}
    for Hkv in (4, 2, 1):
        ops.workspace_for(wl.B, wl.S, wl.D, dev, H, mfma_kv_heads=Hkv)
        variants[f"lanes_Hkv{Hkv}"] = lambda Hkv=Hkv: ops.decode_scan_paged_gqa(wl.q_output, wl.page_table, wl.lengths,
                                                                                wl.attention_result, H, Hkv, 0, 0, wl.elem, wl.S)
        variants[f"mfma_Hkv{Hkv}"] = lambda Hkv=Hkv: ops.decode_scan_paged_gqa_mfma(wl.q_output, wl.page_table, wl.lengths,
                                                                                    wl.attention_result, H, Hkv, 0, wl.S)
    times = timed(variants, args, side)
    base = float(np.median(times["lanes_Hkv8"]))
    out = {"shape": {"dtype": "bf16", "B": wl.B, "S": wl.S, "D": wl.D, "H": H}, "regions": args.regions,
           "launches_per_region": args.launches, "variants": {}}
    for k, t in times.items():
        Hkv = int(k.split("Hkv")[1])
        v = out["variants"][k] = stats(t, live * 2 * (wl.D // H * Hkv) * wl.esize)
        v["time_vs_multi_head"] = round(v["us_median"] / base, 3)
        v["one_over_g"] = round(Hkv / H, 3)
        if k.startswith("mfma"):
            v["time_vs_lane_group"] = round(v["us_median"] / float(np.median(times[f"lanes_Hkv{Hkv}"])), 3)
    return out


def wide(args, dev, side):
    B, S, H, Hkv, hd = 256, 4096, 32, 8, 128
    D, W = H * hd, S // 16
    rng = np.random.default_rng(0x5EED)
    L = rng.integers(S // 4, 3 * S // 4 + 1, size=B).astype(np.int32)
    pool = torch.empty(B * W * 16 * 3 * D, dtype=torch.bfloat16, device=dev).uniform_(-1, 1)
    table = torch.from_numpy((pool.data_ptr() + 2 * 16 * 3 * D * rng.permutation(B * W).astype(np.int64)).reshape(B, W)).to(dev)
    q = torch.rand(B, D, device=dev) * 2 - 1
    out = torch.empty(B, D, device=dev)
    Ld = torch.from_numpy(L).to(dev)
    ops.workspace_for(B, S, D, dev, H, mfma_kv_heads=Hkv)
    n_read = 1 << 30                                    # floats: 4 GiB of the pool, far beyond the 256 MiB Infinity Cache
    stream_src, sink = pool.view(torch.float32)[:n_read], torch.zeros(64, device=dev)
    times = timed({"mfma": lambda: ops.decode_scan_paged_gqa_mfma(q, table, Ld, out, H, Hkv, 0, S),
                   "stream_read": lambda: ops.stream_read(stream_src, sink)}, args, side)
    res = stats(times["mfma"], int(L.astype(np.int64).sum()) * 2 * Hkv * hd * 2)
    ceiling = stats(times["stream_read"], n_read * 4)
    res["of_8_TBps_peak"] = round(res["kv_TBps"] / 8.0, 3)
    res["of_stream_read_ceiling"] = round(res["kv_TBps"] / ceiling["kv_TBps"], 3)
    return {"shape": {"dtype": "bf16", "B": B, "S": S, "D": D, "H": H, "Hkv": Hkv, "lengths": "U[S/4, 3S/4]"}, "mfma": res,
            "stream_read": {"us_median": ceiling["us_median"], "us_min": ceiling["us_min"], "us_max": ceiling["us_max"],
                            "MB": ceiling["kv_MB"], "TBps": ceiling["kv_TBps"]}}


def engine_wide(args):
    from min_llm_inference_amd import engine as eng
    B, S, H, Hkv, hd, V = 256, 4096, 32, 8, 128, 1024
    D = H * hd
    rng = np.random.default_rng(0x5EED)
    u = lambda *shape, scale=1.0: ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)
    sc = 2.0 / np.sqrt(D)
    e = eng.Engine(eng.PAGED_BF16, B, S, D, V, u(V, D), u(S, D, scale=0.5), u(D, D, scale=sc), u(D, D, scale=sc), u(D, D, scale=sc),
                   n_blocks=B * S // 16, n_heads=H, n_kv_heads=Hkv, heads_mfma=True)
    e.set_pipelined(True)
    n_prompt = 0
    for i in range(B):
        toks = rng.integers(0, V - 1, size=int(rng.integers(S // 4, 3 * S // 4 + 1))).astype(np.int32)
        n_prompt += len(toks)
        e.add_item(i, toks)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = e.run()
    wall = time.perf_counter() - t0
    generated = sum(len(t) for t in dict(e.finished()).values()) - n_prompt
    e.close()
    return {"shape": {"kind": "PAGED_BF16", "B": B, "S": S, "D": D, "H": H, "Hkv": Hkv, "n_vocab": V, "prompts": "U[S/4, 3S/4]",
                      "loop": "pipelined"}, "items": int(st.finished), "prompt_tokens": n_prompt, "generated_tokens": int(generated),
            "wall_s": round(wall, 3), "generated_tokens_per_s": round(generated / wall, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-wide", action="store_true")
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    load_library()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)
    out = {}
    with torch.cuda.stream(side):
        out["config4_bf16_H8"] = config4(args, dev, side)
        torch.cuda.empty_cache()
        if not args.no_wide:
            out["wide_32x128_on_8"] = wide(args, dev, side)
    torch.cuda.empty_cache()
    if not args.no_engine:
        out["engine_32x128_on_8"] = engine_wide(args)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
