"""What learned attention-sink logits cost: the kernels with the switch against the kernels without it (whose code object does not
change) at the same shape, on the same pages, in the same process.  The baseline is never the code under test.

  decode scan     mli_decode_scan_paged_sink_logits against mli_decode_scan_paged_gqa, 8 heads on 8 and on 2 K/V heads
    config-4 shape  bf16, B = 1024, S = 4096, D = 512
    config-3 shape  fp32, B = 256, S = 1024, D = 256
  prompt scan     mli_prompt_scan_paged_sink_logits against mli_prompt_scan_paged at tools/prompt_scan_probe.py's shape: 64 rows of
                  1023 prompt tokens (n_sequence 1024), emb_dim 512, 8 heads, bf16 and fp32 pages
  engine          PAGED_BF16, B = 1024, S = 4096, D = 512, H = 8, 2048 items, --engine-pairs times in turn (plain, with logits,
                  plain, ...) in this one process, every run recorded.  The side with the switch takes all -inf logits, under
                  which the kernels give the plain kernels' bits: both sides decode the same tokens in the same iterations
                  (recorded and compared), and the figure compared is us per iteration.

Both calls of a pair read the same bytes with the same load instructions; the switch adds one 4-byte load, one fmaxf, one expf
and one add per thread where a row's final (m, l) is formed, and nothing to the page loop.  HIP events on the launch stream;
after a warm-up, five regions of 20 launches per variant (the prompt scan: one launch per region, it runs for milliseconds), the
variants interleaved region by region; median / min / max of the regions' per-launch time.

  python tools/sink_logits_probe.py [--out profiles/sink_logits_probe.json] [--no-engine] [--regions 5] [--launches 20]
                                    [--engine-pairs 4]"""
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


def learned_logits(H, dev):
    return torch.linspace(-1.0, 1.0, H, device=dev, dtype=torch.float32)


def scan_table(name, dtype, H, kv_heads, args, dev, side):
    """every Hkv of kv_heads is timed plain and with the logits"""
    wl = bench.Workload(name, dev, 0x5EED, headroom=8, dtype=dtype)
    g = torch.Generator(device=dev)
    g.manual_seed(7)
    wl.q_output.copy_(torch.rand(wl.B, wl.D, device=dev, generator=g) * 2 - 1)
    z = learned_logits(H, dev)

    def plain(Hkv):
        return lambda: ops.decode_scan_paged_gqa(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, 0, 0, wl.elem,
                                                 wl.S)

    def sunk(Hkv):
        return lambda: ops.decode_scan_paged_sink_logits(wl.q_output, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, 0, 0,
                                                         z, wl.elem, wl.S)

    variants = {}
    for Hkv in kv_heads:
        variants[f"H{H}_Hkv{Hkv}_plain"] = plain(Hkv)
        variants[f"H{H}_Hkv{Hkv}_sink_logits"] = sunk(Hkv)
    ops.workspace_for(wl.B, wl.S, wl.D, dev, H)   # grown once, before anything is timed
    times = interleaved(variants, args.regions, args.launches, side)
    out = {"shape": {"dtype": dtype, "B": wl.B, "S": wl.S, "D": wl.D, "H": H}, "regions": args.regions,
           "launches_per_region": args.launches, "variants": {k: summary(t) for k, t in times.items()}, "sink_logits_vs_plain": {}}
    for Hkv in kv_heads:
        k = f"H{H}_Hkv{Hkv}"
        out["sink_logits_vs_plain"][k] = round(float(np.median(times[k + "_sink_logits"])) / float(np.median(times[k + "_plain"])), 3)
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
    z = learned_logits(H, dev)
    variants = {
        "plain": lambda: ops.prompt_scan_paged(q, table, None, out, B, S, elem, n_heads=H, seg_arrays=seg_arrays),
        "sink_logits": lambda: ops.prompt_scan_paged(q, table, None, out, B, S, elem, n_heads=H, seg_arrays=seg_arrays, sink_logits=z),
    }
    times = interleaved(variants, args.regions, 1, side, warm=1)
    rec = {"elem": elem_name, "n_heads": H, "tq": ops.prompt_scan_tq(D, H, elem), "queries": B * L,
           "variants": {k: summary(t) for k, t in times.items()},
           "sink_logits_vs_plain": round(float(np.median(times["sink_logits"])) / float(np.median(times["plain"])), 3)}
    del pool
    torch.cuda.empty_cache()
    return rec


def engine_rate(n_heads, sink_logits, dev):
    B, S, D, V = 1024, 4096, 512, bench.N_VOCAB
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * B)]
    e = eng.Engine(eng.PAGED_BF16, B, S, D, V, *weights, n_blocks=B * S // 32, device=dev.index, n_heads=n_heads,
                   sink_logits=sink_logits)
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
        out["config4_bf16"] = scan_table("c4", "bf16", 8, (8, 2), args, dev, side)
        out["config3_f32"] = scan_table("c3", "f32", 8, (8, 2), args, dev, side)
        out["prompt_scan_64x1023_D512_H8"] = [prompt_table(e, 8, args, dev, side) for e in ("bf16", "f32")]
    if not args.no_engine:
        e = out["engine_paged_bf16_B1024_S4096_D512_H8_2048_items"] = {"pairs": args.engine_pairs,
                                                                        "order": "plain, all -inf logits, ..."}
        runs = {"plain": [], "sink_logits_none": []}
        none = [-float("inf")] * 8
        for _ in range(args.engine_pairs):          # in turn, so that a drift of the box falls on both sides alike
            runs["plain"].append(engine_rate(8, None, dev))
            runs["sink_logits_none"].append(engine_rate(8, none, dev))
        for k, rs in runs.items():
            per = [r["us_per_iteration"] for r in rs]
            e[k] = {"tokens_runs": [r["tokens"] for r in rs], "iterations_runs": [r["iterations"] for r in rs],
                    "seconds_runs": [r["seconds"] for r in rs], "us_per_iteration_runs": per,
                    "us_per_iteration_median": round(float(np.median(per)), 1), "us_per_iteration_min": min(per),
                    "us_per_iteration_max": max(per)}
        e["same_tokens_and_iterations"] = len({(r["tokens"], r["iterations"]) for rs in runs.values() for r in rs}) == 1
        e["sink_logits_vs_plain_us_per_iteration_median"] = round(e["sink_logits_none"]["us_per_iteration_median"] /
                                                                  e["plain"]["us_per_iteration_median"], 3)
        e["sink_logits_vs_plain_per_pair"] = [round(c["us_per_iteration"] / p["us_per_iteration"], 3)
                                              for p, c in zip(runs["plain"], runs["sink_logits_none"])]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
