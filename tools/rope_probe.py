"""What the rotary-embedding switch costs the paged projection, the prefill and an engine: every call with a table of all (1, 0)
-- the ROPE instantiations computing the bits of the plain kernels -- against the same call without a table, in one process.

  config 4   bf16, B = 1024, S = 4096, D = 512, 8 heads
  config 3   fp32, B = 256, S = 1024, D = 256, 8 heads: without a table the projection is the panel kernel, with one the tiled
             kernel -- the price of leaving the panel kernel
  e1         bf16, B = 1024, S = 128, D = 2048, 8 heads: without a table the LDS-DMA kernel, with one the tiled kernel -- the price
             of leaving the LDS-DMA kernel
  fp8        config 4 on fp8 pages
  engine     PAGED_BF16, B = 1024, S = 4096, D = 512, 8 heads, 2048 items: without the switch and with the identity table (the
             same tokens: the comparable pair), --engine-pairs times in turn, every run recorded

Per shape: the decode projection (mli_get_latest_k_q_v_paged_lean / _rope) and the prefill of the first --new-rows rows
(mli_paged_prefill / _rope).  --parent-lib names the library built from the parent commit: its plain calls are then timed
beside this build's ("parent" variants), alternating, so that "the switch off costs nothing" is a measurement too.  HIP events
on the launch stream; after a warm-up, --regions regions of --launches launches per variant, the variants interleaved region by
region; median / min / max of the regions' per-launch time, and the ratios of the medians.

  python tools/rope_probe.py [--out profiles/rope_probe.json] [--parent-lib PATH] [--no-engine] [--regions 5] [--launches 20]
                             [--engine-pairs 4] [--new-rows 64]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from min_llm_inference_amd import _lib, engine as eng, load_library, ops  # noqa: E402

H = 8


def region(fn, launches, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(launches):
        fn()
    e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def shape_table(name, dtype, args, dev, side, parent):
    wl = bench.Workload(name, dev, 0x5EED, headroom=8, dtype=dtype)
    B, S, D = wl.B, wl.S, wl.D
    ident = np.zeros((S, D // H // 2, 2), np.float32)
    ident[..., 0] = 1.0
    table = torch.from_numpy(ident).to(dev)
    n_new = min(args.new_rows, B)
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    inp = torch.randint(0, bench.N_VOCAB - 1, (B, S), device=dev, generator=g, dtype=torch.int32)
    new_idx = torch.arange(B, device=dev, dtype=torch.int32)
    st = ctypes.c_void_p(side.cuda_stream)

    # every variant is one ctypes call on prebuilt arguments, so that the host side of a launch is the same on every side
    # (these launches take 7 - 30 us: a Python wrapper's own microseconds would be part of the figure)
    lib = load_library()

    def check(rc):
        assert rc == 0, rc

    pt, ln, wk, wq, wv, qo = (_p(t) for t in (wl.page_table, wl.lengths, wl.wk, wl.wq, wl.wv, wl.q_output))
    emb, wpe, ip, ni, tb = (_p(t) for t in (wl.emb_table, wl.wpe, inp, new_idx, table))

    def latest(which):
        return lambda: check(which.mli_get_latest_k_q_v_paged_lean(pt, ln, wk, wq, wv, qo, B, S, D, wl.elem, st))

    def prefill(which):
        return lambda: check(which.mli_paged_prefill(emb, wpe, ip, pt, ln, ni, wk, wv, B, S, D, n_new, wl.elem, st))

    variants = {"latest_plain": latest(lib),
                "latest_identity_table": lambda: check(lib.mli_get_latest_k_q_v_paged_rope(pt, ln, wk, wq, wv, qo, B, S, D, H, tb,
                                                                                            wl.elem, st)),
                "prefill_plain": prefill(lib),
                "prefill_identity_table": lambda: check(lib.mli_paged_prefill_rope(emb, wpe, ip, pt, ln, ni, wk, wv, B, S, D, n_new, 0,
                                                                                   0, H, tb, wl.elem, st))}
    if parent is not None:   # the parent commit's library: the same plain calls
        variants["latest_parent"] = latest(parent)
        variants["prefill_parent"] = prefill(parent)
    # which kernels ran, by the launch counters, and that the identity table gives the plain call's bits
    families = {}
    for k in ("latest_plain", "latest_identity_table", "prefill_plain", "prefill_identity_table"):
        load_library().mli_launch_counts_reset()
        variants[k]()
        families[k] = {f: ops.launch_count(f) for f in ("gemm_f32_panel", "gemm_f32_rows64", "gemm_f32_rows64_split", "gemm_f32_rows128",
                                                        "gemm_bf16_rows64", "gemm_bf16_deep", "gemm_bf16_rows128", "gemm_bf16_dma",
                                                        "gemm_bf16_fill", "gemm_f32_rope", "gemm_bf16_rope", "prefill_fused",
                                                        "prefill_two_launch") if ops.launch_count(f)}
    variants["latest_plain"]()
    side.synchronize()
    q_plain = wl.q_output.clone()
    variants["latest_identity_table"]()
    side.synchronize()
    same_bits = bool(torch.equal(q_plain.view(torch.int32), wl.q_output.view(torch.int32)))
    times = {k: [] for k in variants}
    for fn in variants.values():
        for _ in range(5):
            fn()
    side.synchronize()
    for _ in range(args.regions):
        for k, fn in variants.items():
            times[k].append(region(fn, args.launches, side))
    out = {"shape": {"dtype": dtype, "B": B, "S": S, "D": D, "H": H, "prefill_new_rows": n_new,
                     "prefill_tokens": int(wl.lengths_host[:n_new].sum())},
           "regions": args.regions, "launches_per_region": args.launches, "kernels": families,
           "identity_table_q_bits_equal_plain": same_bits, "variants": {}, "ratios_of_medians": {}}
    med = {k: float(np.median(t)) for k, t in times.items()}
    for k, t in times.items():
        out["variants"][k] = {"us_median": round(med[k], 2), "us_min": round(min(t), 2), "us_max": round(max(t), 2)}
    for what in ("latest", "prefill"):
        out["ratios_of_medians"][f"{what}_identity_table_vs_plain"] = round(med[f"{what}_identity_table"] / med[f"{what}_plain"], 3)
        if parent is not None:
            out["ratios_of_medians"][f"{what}_plain_vs_parent"] = round(med[f"{what}_plain"] / med[f"{what}_parent"], 3)
    del wl
    torch.cuda.empty_cache()
    return out


def engine_rate(rope, dev):
    B, S, D, V = 1024, 4096, 512, bench.N_VOCAB
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * B)]
    e = eng.Engine(eng.PAGED_BF16, B, S, D, V, *weights, n_blocks=B * S // 32, device=dev.index, n_heads=H, rope=rope)
    for i, toks in items:
        e.add_item(i, toks)
    st = e.run()
    e.close()
    assert st.finished == 2 * B
    return {"tokens": int(st.total_tokens), "seconds": round(st.seconds, 3), "iterations": int(st.iterations)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--engine-pairs", type=int, default=4)
    ap.add_argument("--new-rows", type=int, default=64)
    args = ap.parse_args()
    load_library()
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        for name in ("mli_get_latest_k_q_v_paged_lean", "mli_paged_prefill"):
            getattr(parent, name).argtypes = _lib.SIGNATURES[name]
            getattr(parent, name).restype = ctypes.c_int
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)
    out = {"parent_library_timed": parent is not None}
    with torch.cuda.stream(side):
        out["config4_bf16"] = shape_table("c4", "bf16", args, dev, side, parent)
        out["config3_f32"] = shape_table("c3", "f32", args, dev, side, parent)
        out["e1_bf16"] = shape_table("e1", "bf16", args, dev, side, parent)
        out["config4_fp8"] = shape_table("c4", "fp8", args, dev, side, parent)
    if not args.no_engine:
        e = out["engine_paged_bf16_B1024_S4096_D512_H8_2048_items"] = {"pairs": args.engine_pairs, "order": "plain, identity, ..."}
        ident = np.zeros((4096, 512 // H // 2, 2), np.float32)
        ident[..., 0] = 1.0
        runs = {"plain": [], "identity_table": []}
        for _ in range(args.engine_pairs):          # in turn, so that a drift of the box falls on both sides alike
            runs["plain"].append(engine_rate(None, dev))
            runs["identity_table"].append(engine_rate(ident, dev))
        for k, rs in runs.items():
            assert len({(r["tokens"], r["iterations"]) for r in runs["plain"] + rs}) == 1, "the pair decodes the same tokens"
            secs = [r["seconds"] for r in rs]
            e[k] = {"tokens": rs[0]["tokens"], "iterations": rs[0]["iterations"], "seconds_runs": secs,
                    "seconds_median": round(float(np.median(secs)), 3), "seconds_min": min(secs), "seconds_max": max(secs)}
        e["identity_vs_plain_seconds_median"] = round(e["identity_table"]["seconds_median"] / e["plain"]["seconds_median"], 3)
        e["identity_vs_plain_per_pair"] = [round(z["seconds"] / p["seconds"], 3) for p, z in zip(runs["plain"], runs["identity_table"])]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
