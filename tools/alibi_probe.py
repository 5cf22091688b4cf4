"""What ALiBi costs the lean paged scan: mli_decode_scan_paged_alibi (standard slopes) against mli_decode_scan_paged_gqa (the
existing kernels, whose code object does not change) at the same shape, on the same pages, in the same process.

  config-4 shape  bf16, B = 1024, S = 4096, D = 512, H = 8: Hkv = 8 (g 1) and Hkv = 2 (g 4), without a window and with W = 1024
  config-3 shape  fp32, B = 256, S = 1024, D = 256, H = 4, Hkv = 4, without a window
  engine          PAGED_BF16, B = 1024, S = 4096, D = 512, H = 8, 2048 items: without the switch and with slopes all zero (the
                  ALiBi kernels on the same tokens: the comparable pair), --engine-pairs times in turn (plain, zero, plain,
                  zero, ...) in this one process, every run recorded, median / min / max of each side and the ratio of the
                  medians; once with the standard slopes (another model: it decodes other tokens and other stream lengths, so
                  its rate says nothing about the kernel)

Both calls read the same bytes with the same load instructions; the bias is one fmaf per score.  Reported per pair: us per
launch of each and alibi / plain.  HIP events on the launch stream; after a warm-up, five regions of 20 launches per variant,
the variants interleaved region by region; median / min / max of the regions' per-launch time.

  python tools/alibi_probe.py [--out profiles/alibi_probe.json] [--no-engine] [--regions 5] [--launches 20] [--engine-pairs 4]"""
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


def region(fn, launches, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        fn()
    e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us


def scan_table(name, dtype, H, forms, args, dev, side):
    """forms: (Hkv, W) pairs; every pair is timed plain and with the bias"""
    wl = bench.Workload(name, dev, 0x5EED, headroom=8, dtype=dtype)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    wl.q_output.copy_(torch.rand(wl.B, wl.D, device=dev, generator=g) * 2 - 1)
    slopes = torch.from_numpy(ops.alibi_slopes(H)).to(dev)

    def plain(Hkv, W):
        return lambda: ops.decode_scan_paged_gqa(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, W, 0,
                                                 wl.elem, wl.S)

    def alibi(Hkv, W):
        return lambda: ops.decode_scan_paged_alibi(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, W, 0,
                                                   slopes, wl.elem, wl.S)

    variants = {}
    for Hkv, W in forms:
        variants[f"H{H}_Hkv{Hkv}_W{W or '-'}_plain"] = plain(Hkv, W)
        variants[f"H{H}_Hkv{Hkv}_W{W or '-'}_alibi"] = alibi(Hkv, W)
    ops.workspace_for(wl.B, wl.S, wl.D, dev, H)   # grown once, before anything is timed
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(5):
            fn()
    side.synchronize()
    for _ in range(args.regions):
        for k, fn in variants.items():
            times[k].append(region(fn, args.launches, side))
    out = {"shape": {"dtype": dtype, "B": wl.B, "S": wl.S, "D": wl.D, "H": H}, "regions": args.regions,
           "launches_per_region": args.launches, "variants": {}, "alibi_vs_plain": {}}
    for k, t in times.items():
        out["variants"][k] = {"us_median": round(float(np.median(t)), 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1)}
    for Hkv, W in forms:
        k = f"H{H}_Hkv{Hkv}_W{W or '-'}"
        out["alibi_vs_plain"][k] = round(float(np.median(times[k + "_alibi"])) / float(np.median(times[k + "_plain"])), 3)
    del wl
    torch.cuda.empty_cache()
    return out


def engine_rate(n_heads, alibi, dev):
    B, S, D, V = 1024, 4096, 512, bench.N_VOCAB
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * B)]
    e = eng.Engine(eng.PAGED_BF16, B, S, D, V, *weights, n_blocks=B * S // 32, device=dev.index, n_heads=n_heads,
                   alibi=alibi)
    for i, toks in items:
        e.add_item(i, toks)
    st = e.run()
    e.close()
    assert st.finished == 2 * B
    return {"tokens": int(st.total_tokens), "seconds": round(st.seconds, 3), "iterations": int(st.iterations),
            "tokens_per_s": round(st.total_tokens / st.seconds, 1),
            "us_per_iteration": round(1e6 * st.seconds / max(int(st.iterations), 1), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--engine-pairs", type=int, default=4)
    args = ap.parse_args()
    load_library()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)
    out = {}
    with torch.cuda.stream(side):
        out["config4_bf16"] = scan_table("c4", "bf16", 8, ((8, 0), (2, 0), (8, 1024), (2, 1024)), args, dev, side)
        out["config3_f32"] = scan_table("c3", "f32", 4, ((4, 0),), args, dev, side)
    if not args.no_engine:
        e = out["engine_paged_bf16_B1024_S4096_D512_H8_2048_items"] = {"pairs": args.engine_pairs, "order": "plain, zero, ..."}
        runs = {"plain": [], "alibi_zero_slopes": []}
        for _ in range(args.engine_pairs):          # in turn, so that a drift of the box falls on both sides alike
            runs["plain"].append(engine_rate(8, None, dev))
            runs["alibi_zero_slopes"].append(engine_rate(8, (0.0,) * 8, dev))
        for k, rs in runs.items():
            assert len({(r["tokens"], r["iterations"]) for r in runs["plain"] + rs}) == 1, "the pair decodes the same tokens"
            secs = [r["seconds"] for r in rs]
            e[k] = {"tokens": rs[0]["tokens"], "iterations": rs[0]["iterations"], "seconds_runs": secs,
                    "seconds_median": round(float(np.median(secs)), 3), "seconds_min": min(secs), "seconds_max": max(secs)}
        e["zero_slopes_vs_plain_seconds_median"] = round(e["alibi_zero_slopes"]["seconds_median"] / e["plain"]["seconds_median"], 3)
        e["zero_slopes_vs_plain_per_pair"] = [round(z["seconds"] / p["seconds"], 3)
                                              for p, z in zip(runs["plain"], runs["alibi_zero_slopes"])]
        e["alibi_standard_slopes"] = engine_rate(8, True, dev)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
