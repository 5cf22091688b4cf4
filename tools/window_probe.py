"""What a sliding window costs and gains the lean paged scan (mli_decode_scan_paged_window), and what attention sinks
(mli_decode_scan_paged_sinks) cost beside it, on the same pages, in the same process.

  config-4 shape  bf16, B = 1024, S = 4096, D = 512, lengths U[S/4, 3S/4]
  config-3 shape  fp32, B = 256, S = 1024, D = 256 (W = 1024 is "no window" there: the un-windowed kernels)
  per shape, W in {256, 1024} and H in {1, 8}:
    H{H}_W{W}        the windowed scan on the true lengths
    H{H}_base_W{W}   the un-windowed lean chunked scan (H = 1: scan_stream 0; H = 8: the multi-head scan) with the lengths
                     replaced by min(L, W): the same bytes to within 15 tokens a row, no window logic.  time / this = the PRICE
    H{H}_full        the un-windowed scan on the true lengths, as a caller gets it by default.  time / this = the GAIN
    H{H}_W{W}_K4     the windowed scan with 4 sinks on the true lengths: one more page a row (the sink page), the two-run page
                     mapping and the second mask.  time / H{H}_W{W} = what the sinks cost (where K + W >= S, config-3 shape
                     at W = 1024, both are the un-windowed kernels)
  engine          PAGED_BF16, B = 1024, S = 4096, D = 512, 2048 items, window 1024 against none, tokens/s

TB/s is on the bytes the window leaves, sum of 2 min(L, W) D e (with sinks: 2 min(L, W + K) D e).  HIP events on the launch
stream; after a warm-up, five regions of >= 20 launches per variant, the variants interleaved region by region; median /
min / max of the regions' per-launch time.

  python tools/window_probe.py [--out profiles/window_probe.json] [--no-engine] [--regions 5] [--launches 20]
Under rocprofv3 --kernel-trace --stats use --no-engine --regions 1."""
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

WINDOWS = (256, 1024)
HEADS = (1, 8)
SINKS = 4


def region(fn, launches, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        fn()
    e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us


def scan_table(lib, name, dtype, args, dev, side):
    wl = bench.Workload(name, dev, 0x5EED, headroom=8, dtype=dtype)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    wl.q_output.copy_(torch.rand(wl.B, wl.D, device=dev, generator=g) * 2 - 1)
    cut = {W: torch.clamp(wl.lengths, max=W) for W in WINDOWS}
    kv_bytes = {W: int(2 * np.minimum(wl.lengths_host, W).astype(np.int64).sum() * wl.D * wl.esize) for W in WINDOWS}
    kv_full = int(2 * wl.lengths_host.astype(np.int64).sum() * wl.D * wl.esize)
    kv_sinks = {W: int(2 * np.minimum(wl.lengths_host, W + SINKS).astype(np.int64).sum() * wl.D * wl.esize) for W in WINDOWS}

    def plain(lengths, H):
        if H == 1:
            return lambda: ops.decode_scan_paged(wl.q_output, wl.page_table, lengths, None, wl.attention_result, wl.elem,
                                                 phases=7, n_sequence=wl.S)
        return lambda: ops.decode_scan_paged_heads(wl.q_output, wl.page_table, lengths, wl.attention_result, H, wl.elem, wl.S)

    def windowed(H, W):
        return lambda: ops.decode_scan_paged_window(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, W, wl.elem,
                                                    wl.S)

    def with_sinks(H, W):
        return lambda: ops.decode_scan_paged_sinks(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, W, SINKS,
                                                   wl.elem, wl.S)

    # name -> (scan_stream setting, set once before the variant's launches and never inside a timed region; launch; bytes)
    variants = {}
    for H in HEADS:
        variants[f"H{H}_full"] = (1, plain(wl.lengths, H), kv_full)
        for W in WINDOWS:
            variants[f"H{H}_W{W}"] = (1, windowed(H, W), kv_bytes[W])
            variants[f"H{H}_base_W{W}"] = (0, plain(cut[W], H), kv_bytes[W])
            variants[f"H{H}_W{W}_K{SINKS}"] = (1, with_sinks(H, W), kv_sinks[W])
    ops.workspace_for(wl.B, wl.S, wl.D, dev, max(HEADS))   # grown once, before anything is timed
    times = {k: [] for k in variants}
    try:
        for stream_kernel, fn, _ in variants.values():
            lib.mli_tune(b"scan_stream", stream_kernel)
            for _ in range(5):
                fn()
        side.synchronize()
        for _ in range(args.regions):
            for k, (stream_kernel, fn, _) in variants.items():
                lib.mli_tune(b"scan_stream", stream_kernel)
                times[k].append(region(fn, args.launches, side))
    finally:
        lib.mli_tune(b"scan_stream", 1)
    med = {k: float(np.median(t)) for k, t in times.items()}
    out = {"shape": {"dtype": dtype, "B": wl.B, "S": wl.S, "D": wl.D}, "kv_MB_full": round(kv_full / 1e6, 1),
           "kv_MB_in_window": {str(W): round(kv_bytes[W] / 1e6, 1) for W in WINDOWS},
           "kv_MB_in_window_and_sinks": {str(W): round(kv_sinks[W] / 1e6, 1) for W in WINDOWS}, "n_sink": SINKS,
           "regions": args.regions, "launches_per_region": args.launches, "variants": {}}
    for k, t in times.items():
        row = {"us_median": round(med[k], 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
               "TBps": round(variants[k][2] / med[k] / 1e6, 3)}
        if k.endswith(f"_K{SINKS}"):
            row["time_vs_window"] = round(med[k] / med[k[:-len(f"_K{SINKS}")]], 3)
        elif "_W" in k and "_base_" not in k:
            H, W = k.split("_W")
            row["price_time_vs_base"] = round(med[k] / med[f"{H}_base_W{W}"], 3)
            row["gain_time_vs_full"] = round(med[k] / med[f"{H}_full"], 3)
        out["variants"][k] = row
    del wl
    torch.cuda.empty_cache()
    return out


def engine_rate(window, dev):
    B, S, D, V = 1024, 4096, 512, bench.N_VOCAB
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * B)]
    e = eng.Engine(eng.PAGED_BF16, B, S, D, V, *weights, n_blocks=B * S // 32, device=dev.index, window=window)
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
    lib = load_library()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)
    out = {}
    with torch.cuda.stream(side):
        out["config4_bf16"] = scan_table(lib, "c4", "bf16", args, dev, side)
        out["config3_f32"] = scan_table(lib, "c3", "f32", args, dev, side)
    if not args.no_engine:
        e = {"no_window": engine_rate(None, dev), "W1024": engine_rate(1024, dev)}
        e["W1024_vs_no_window_tokens_per_s"] = round(e["W1024"]["tokens_per_s"] / e["no_window"]["tokens_per_s"], 3)
        out["engine_paged_bf16_B1024_S4096_D512_2048_items"] = e
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
