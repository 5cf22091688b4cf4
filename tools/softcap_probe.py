"""What logit soft-capping costs: the capped kernels against the kernels without the cap (whose code object does not change) at
the same shape, on the same pages, in the same process.  The baseline is never the code under test.

  decode scan     mli_decode_scan_paged_softcap (cap 30) against mli_decode_scan_paged_gqa
    config-4 shape  bf16, B = 1024, S = 4096, D = 512, H = 8: Hkv = 8 (g 1) and Hkv = 2 (g 4), without a window and with W = 1024
    config-3 shape  fp32, B = 256, S = 1024, D = 256, H = 4, Hkv = 4, without a window
  prompt scan     mli_prompt_scan_paged_softcap against mli_prompt_scan_paged at tools/prompt_scan_probe.py's shape: 64 rows of
                  1023 prompt tokens (n_sequence 1024), emb_dim 512, 8 heads, bf16 and fp32 pages
  engine          PAGED_BF16, B = 1024, S = 4096, D = 512, H = 8, 2048 items, --engine-pairs times in turn (plain, capped, plain,
                  capped, ...) in this one process, every run recorded.  There is no cap that gives the plain engine's bits; the
                  capped side takes cap 1e6, under which cap * tanh(x / cap) is x to an ulp, so the pair decodes (nearly) the
                  same streams: tokens and iterations of every run are recorded, and the figure compared is us per iteration.
                  Once with cap 30 (another model: other tokens, other stream lengths; its rate says nothing about the kernel).

Both calls of a pair read the same bytes with the same load instructions; the cap is about twenty VALU instructions per score.
HIP events on the launch stream; after a warm-up, five regions of 20 launches per variant (the prompt scan: one launch per
region, it runs for milliseconds), the variants interleaved region by region; median / min / max of the regions' per-launch time.

  python tools/softcap_probe.py [--out profiles/softcap_probe.json] [--no-engine] [--regions 5] [--launches 20] [--engine-pairs 4]"""
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

CAP, NEUTRAL_CAP = 30.0, 1.0e6


def region(fn, launches, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        fn()
    e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us


def interleaved(variants, regions, launches, stream, warm=5):
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(warm):
            fn()
    stream.synchronize()
    for _ in range(regions):
        for k, fn in variants.items():
            times[k].append(region(fn, launches, stream))
    return times


def summary(t):
    return {"us_median": round(float(np.median(t)), 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1)}


def scan_table(name, dtype, H, forms, args, dev, side):
    """forms: (Hkv, W) pairs; every pair is timed plain and with the cap"""
    wl = bench.Workload(name, dev, 0x5EED, headroom=8, dtype=dtype)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    wl.q_output.copy_(torch.rand(wl.B, wl.D, device=dev, generator=g) * 2 - 1)

    def plain(Hkv, W):
        return lambda: ops.decode_scan_paged_gqa(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, W, 0,
                                                 wl.elem, wl.S)

    def capped(Hkv, W):
        return lambda: ops.decode_scan_paged_softcap(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, W, 0,
                                                     CAP, wl.elem, wl.S)

    variants = {}
    for Hkv, W in forms:
        variants[f"H{H}_Hkv{Hkv}_W{W or '-'}_plain"] = plain(Hkv, W)
        variants[f"H{H}_Hkv{Hkv}_W{W or '-'}_softcap"] = capped(Hkv, W)
    ops.workspace_for(wl.B, wl.S, wl.D, dev, H)   # grown once, before anything is timed
    times = interleaved(variants, args.regions, args.launches, side)
    out = {"shape": {"dtype": dtype, "B": wl.B, "S": wl.S, "D": wl.D, "H": H}, "cap": CAP, "regions": args.regions,
           "launches_per_region": args.launches, "variants": {k: summary(t) for k, t in times.items()}, "softcap_vs_plain": {}}
    for Hkv, W in forms:
        k = f"H{H}_Hkv{Hkv}_W{W or '-'}"
        out["softcap_vs_plain"][k] = round(float(np.median(times[k + "_softcap"])) / float(np.median(times[k + "_plain"])), 3)
    del wl
    torch.cuda.empty_cache()
    return out


def prompt_table(elem_name, H, args, dev, side):
    """tools/prompt_scan_probe.py's pages and queries: one segment of 1023 positions per row"""
    B, S, D, L = 64, 1024, 512, 1023
    elem = {"f32": 0, "bf16": 1}[elem_name]
    dtype = torch.float32 if elem == 0 else torch.bfloat16
    esize = 4 if elem == 0 else 2
    g = torch.Generator(device=dev)
    g.manual_seed(11 + H)
    n_pages = B * S // 16
    pool = ((torch.rand(n_pages * 16 * 3 * D, device=dev, generator=g) * 2 - 1) / 8).to(dtype)
    order = torch.randperm(n_pages, generator=torch.Generator().manual_seed(3)).numpy().astype(np.int64)
    table = torch.from_numpy((pool.data_ptr() + order * 16 * 3 * D * esize).reshape(B, S // 16)).to(dev)
    q = torch.rand(B * L, D, device=dev, generator=g) * 2 - 1
    out = torch.empty(B * L, D, device=dev)
    arrays, max_count, _ = ops._segments([(b, 0, L) for b in range(B)], dev)
    seg_arrays = (*arrays, max_count)
    variants = {
        "plain": lambda: ops.prompt_scan_paged(q, table, None, out, B, S, elem, n_heads=H, seg_arrays=seg_arrays),
        "softcap": lambda: ops.prompt_scan_paged(q, table, None, out, B, S, elem, n_heads=H, seg_arrays=seg_arrays, softcap=CAP),
    }
    times = interleaved(variants, args.regions, 1, side, warm=1)
    rec = {"elem": elem_name, "n_heads": H, "tq": ops.prompt_scan_tq(D, H, elem), "queries": B * L, "cap": CAP,
           "variants": {k: summary(t) for k, t in times.items()},
           "softcap_vs_plain": round(float(np.median(times["softcap"])) / float(np.median(times["plain"])), 3)}
    del pool
    torch.cuda.empty_cache()
    return rec


def engine_rate(n_heads, softcap, dev):
    B, S, D, V = 1024, 4096, 512, bench.N_VOCAB
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * B)]
    e = eng.Engine(eng.PAGED_BF16, B, S, D, V, *weights, n_blocks=B * S // 32, device=dev.index, n_heads=n_heads, softcap=softcap)
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
        out["prompt_scan_64x1023_D512_H8"] = [prompt_table(e, 8, args, dev, side) for e in ("bf16", "f32")]
    if not args.no_engine:
        e = out["engine_paged_bf16_B1024_S4096_D512_H8_2048_items"] = {"pairs": args.engine_pairs, "order": "plain, capped, ...",
                                                                        "neutral_cap": NEUTRAL_CAP}
        runs = {"plain": [], "softcap_neutral": []}
        for _ in range(args.engine_pairs):          # in turn, so that a drift of the box falls on both sides alike
            runs["plain"].append(engine_rate(8, None, dev))
            runs["softcap_neutral"].append(engine_rate(8, NEUTRAL_CAP, dev))
        for k, rs in runs.items():
            per = [r["us_per_iteration"] for r in rs]
            e[k] = {"tokens_runs": [r["tokens"] for r in rs], "iterations_runs": [r["iterations"] for r in rs],
                    "seconds_runs": [r["seconds"] for r in rs], "us_per_iteration_runs": per,
                    "us_per_iteration_median": round(float(np.median(per)), 1), "us_per_iteration_min": min(per),
                    "us_per_iteration_max": max(per)}
        e["same_tokens_and_iterations"] = len({(r["tokens"], r["iterations"]) for rs in runs.values() for r in rs}) == 1
        e["softcap_vs_plain_us_per_iteration_median"] = round(e["softcap_neutral"]["us_per_iteration_median"] /
                                                              e["plain"]["us_per_iteration_median"], 3)
        e["softcap_vs_plain_per_pair"] = [round(c["us_per_iteration"] / p["us_per_iteration"], 3)
                                          for p, c in zip(runs["plain"], runs["softcap_neutral"])]
        e["softcap_cap_30"] = engine_rate(8, CAP, dev)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
