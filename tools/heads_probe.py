"""What per-head softmax state costs the lean paged scan: the multi-head scan (mli_decode_scan_paged_heads) against the
single-head scans at the same shape, on the same pages, in the same process.

  config-4 shape  bf16, B = 1024, S = 4096, D = 512: H = 1 on the chunked grid (scan_stream 0) and on the equal-shares
                  kernel, H = 4, 8, 16
  config-3 shape  fp32, B = 256, S = 1024, D = 256: H = 1 (chunked grid), 2, 4, 8
  engine          PAGED_BF16, B = 1024, S = 4096, D = 512, 2048 items, H = 8 against H = 1, tokens/s

Every variant reads the same algorithmic bytes (sum of 2 L D e), so time ratios are the price of the per-head state.  HIP
events on the launch stream; after a warm-up, five regions of >= 20 launches per variant, the variants interleaved region by
region; median / min / max of the regions' per-launch time.

  python tools/heads_probe.py [--out profiles/heads_probe.json] [--no-engine] [--regions 5] [--launches 20]
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


def region(fn, launches, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        fn()
    e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us


def scan_table(lib, name, dtype, heads, with_stream, args, dev, side):
    wl = bench.Workload(name, dev, 0x5EED, headroom=8, dtype=dtype)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    wl.q_output.copy_(torch.rand(wl.B, wl.D, device=dev, generator=g) * 2 - 1)
    alg = wl.algorithmic_bytes(wl.lengths_host)["scan_lean"]

    def single():
        ops.decode_scan_paged(wl.q_output, wl.page_table, wl.lengths, None, wl.attention_result, wl.elem, phases=7,
                              n_sequence=wl.S)

    def multi(H):
        return lambda: ops.decode_scan_paged_heads(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, wl.elem,
                                                   wl.S)

    # name -> (scan_stream setting, set once before the variant's launches and never inside a timed region; launch)
    variants = {"H1_chunked": (0, single)}
    if with_stream:
        variants["H1_equal_shares"] = (1, single)
    for H in heads:
        variants[f"H{H}"] = (0, multi(H))   # (the key does not apply to the multi-head scan)
    ops.workspace_for(wl.B, wl.S, wl.D, dev, max(heads))   # grown once, before anything is timed
    times = {k: [] for k in variants}
    try:
        for stream_kernel, fn in variants.values():
            lib.mli_tune(b"scan_stream", stream_kernel)
            for _ in range(5):
                fn()
        side.synchronize()
        for _ in range(args.regions):
            for k, (stream_kernel, fn) in variants.items():
                lib.mli_tune(b"scan_stream", stream_kernel)
                times[k].append(region(fn, args.launches, side))
    finally:
        lib.mli_tune(b"scan_stream", 1)
    base = float(np.median(times["H1_chunked"]))
    out = {"shape": {"dtype": dtype, "B": wl.B, "S": wl.S, "D": wl.D}, "algorithmic_MB": round(alg / 1e6, 1),
           "regions": args.regions, "launches_per_region": args.launches, "variants": {}}
    for k, t in times.items():
        med = float(np.median(t))
        out["variants"][k] = {"us_median": round(med, 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                              "TBps": round(alg / med / 1e6, 3), "time_vs_H1_chunked": round(med / base, 3)}
    del wl
    torch.cuda.empty_cache()
    return out


def engine_rate(n_heads, dev):
    B, S, D, V = 1024, 4096, 512, bench.N_VOCAB
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * B)]
    e = eng.Engine(eng.PAGED_BF16, B, S, D, V, *weights, n_blocks=B * S // 32, device=dev.index, n_heads=n_heads)
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
        out["config4_bf16"] = scan_table(lib, "c4", "bf16", (4, 8, 16), True, args, dev, side)
        out["config3_f32"] = scan_table(lib, "c3", "f32", (2, 4, 8), False, args, dev, side)
    if not args.no_engine:
        out["engine_paged_bf16_B1024_S4096_D512_2048_items"] = {f"H{H}": engine_rate(H, dev) for H in (1, 8)}
        e = out["engine_paged_bf16_B1024_S4096_D512_2048_items"]
        e["H8_vs_H1_tokens_per_s"] = round(e["H8"]["tokens_per_s"] / e["H1"]["tokens_per_s"], 3)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
