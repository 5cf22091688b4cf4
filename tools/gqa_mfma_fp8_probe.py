"""The grouped-query scan on matrix instructions over fp8 pages (mli_decode_scan_paged_gqa_mfma_fp8) timed on an
MI355X against the bf16 kernel (mli_decode_scan_paged_gqa_mfma, unchanged) on the same lengths, in alternated regions.

  (a) config-4 shape  B = 1024, S = 4096, D = 512, H = 8, ragged lengths, Hkv = 4 / 2 / 1 (g = 2 / 4 / 8): bf16 pages | fp8 pages
  (b) wide shape      B = 512, S = 4096, 16 heads of 128 on 4 K/V heads (D = 2048, the widest fp8 row), lengths U[S/4, 3S/4]: the
      2048 virtual rows of the bf16 kernel's published shape (B = 256, 32 heads on 8, which is beyond the fp8 emb_dim limit);
      K/V bytes per second of both against the streaming-read rate (mli_stream_read, 4 GiB per launch) of the same run
  (c) end to end      the PAGED_FP8 and the PAGED_BF16 engine at B = 256 of that shape (gqa_mfma_probe.engine_wide's workload):
      generated tokens per second of wall time of one run each, prefill included

HIP events on the launch stream; after a warm-up, --regions regions of --launches launches per variant, interleaved region by
region; median / min / max of the regions' per-launch time (gqa_mfma_probe.timed).

  python tools/gqa_mfma_fp8_probe.py [--out profiles/gqa_mfma_fp8_probe.json] [--regions 7] [--launches 20] [--no-engine]"""
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
from gqa_mfma_probe import stats, timed  # noqa: E402
from min_llm_inference_amd import load_library, ops  # noqa: E402

SCAN = {"bf16": ops.decode_scan_paged_gqa_mfma, "fp8": ops.decode_scan_paged_gqa_mfma_fp8}


def pair(res):
    res["fp8"]["time_vs_bf16"] = round(res["fp8"]["us_median"] / res["bf16"]["us_median"], 3)
    return res


def config4(args, dev, side):
    H, out = 8, {}
    wls = {dt: bench.Workload("c4", dev, 0x5EED, headroom=8, dtype=dt) for dt in SCAN}
    wl = wls["bf16"]
    assert np.array_equal(np.asarray(wl.lengths_host), np.asarray(wls["fp8"].lengths_host))
    q = torch.rand(wl.B, wl.D, device=dev) * 2 - 1
    live = int(np.minimum(np.asarray(wl.lengths_host).astype(np.int64), wl.S).sum())
    for Hkv in (4, 2, 1):
        ops.workspace_for(wl.B, wl.S, wl.D, dev, H, mfma_kv_heads=Hkv)
        times = timed({dt: lambda dt=dt: SCAN[dt](q, wls[dt].page_table, wls[dt].lengths, wls[dt].attention_result, H, Hkv, 0, wl.S)
                       for dt in SCAN}, args, side)
        out[f"Hkv{Hkv}"] = pair({dt: stats(times[dt], live * 2 * (wl.D // H * Hkv) * wls[dt].esize) for dt in SCAN})
    return {"shape": {"B": wl.B, "S": wl.S, "D": wl.D, "H": H}, "regions": args.regions, "launches_per_region": args.launches, **out}


def wide(args, dev, side):
    B, S, H, Hkv, hd = 512, 4096, 16, 4, 128
    D, W = H * hd, S // 16
    rng = np.random.default_rng(0x5EED)
    L = rng.integers(S // 4, 3 * S // 4 + 1, size=B).astype(np.int32)
    order = rng.permutation(B * W).astype(np.int64)
    pools = {"bf16": torch.empty(B * W * 16 * 3 * D, dtype=torch.bfloat16, device=dev).uniform_(-1, 1)}
    pools["fp8"] = torch.empty(B * W * 16 * 3 * D, dtype=torch.uint8, device=dev)
    chunk = 1 << 26
    for o in range(0, pools["fp8"].numel(), chunk):
        ops.f32_to_fp8(pools["bf16"][o:o + chunk].float(), pools["fp8"][o:o + chunk])
    esize = {"bf16": 2, "fp8": 1}
    tables = {dt: torch.from_numpy((p.data_ptr() + esize[dt] * 16 * 3 * D * order).reshape(B, W)).to(dev) for dt, p in pools.items()}
    q = torch.rand(B, D, device=dev) * 2 - 1
    out = torch.empty(B, D, device=dev)
    Ld = torch.from_numpy(L).to(dev)
    ops.workspace_for(B, S, D, dev, H, mfma_kv_heads=Hkv)
    n_read = 1 << 30                                    # floats: 4 GiB of the bf16 pool, far beyond the 256 MiB Infinity Cache
    stream_src, sink = pools["bf16"].view(torch.float32)[:n_read], torch.zeros(64, device=dev)
    variants = {dt: lambda dt=dt: SCAN[dt](q, tables[dt], Ld, out, H, Hkv, 0, S) for dt in SCAN}
    variants["stream_read"] = lambda: ops.stream_read(stream_src, sink)
    times = timed(variants, args, side)
    ceiling = stats(times["stream_read"], n_read * 4)
    res = pair({dt: stats(times[dt], int(L.astype(np.int64).sum()) * 2 * Hkv * hd * esize[dt]) for dt in SCAN})
    for dt in SCAN:
        res[dt]["of_stream_read_rate"] = round(res[dt]["kv_TBps"] / ceiling["kv_TBps"], 3)
    return {"shape": {"B": B, "S": S, "D": D, "H": H, "Hkv": Hkv, "lengths": "U[S/4, 3S/4]"}, **res,
            "stream_read": {"us_median": ceiling["us_median"], "MB": ceiling["kv_MB"], "TBps": ceiling["kv_TBps"]}}


def engine_wide(kind_name):
    from min_llm_inference_amd import engine as eng
    B, S, H, Hkv, hd, V = 256, 4096, 16, 4, 128, 1024
    D = H * hd
    rng = np.random.default_rng(0x5EED)
    u = lambda *shape, scale=1.0: ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)
    sc = 2.0 / np.sqrt(D)
    e = eng.Engine(getattr(eng, kind_name), B, S, D, V, u(V, D), u(S, D, scale=0.5), u(D, D, scale=sc), u(D, D, scale=sc),
                   u(D, D, scale=sc), n_blocks=B * S // 16, n_heads=H, n_kv_heads=Hkv, heads_mfma=True)
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
    return {"shape": {"kind": kind_name, "B": B, "S": S, "D": D, "H": H, "Hkv": Hkv, "n_vocab": V, "loop": "pipelined"},
            "items": int(st.finished), "prompt_tokens": n_prompt, "generated_tokens": int(generated), "wall_s": round(wall, 3),
            "generated_tokens_per_s": round(generated / wall, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--no-engine", action="store_true")
    args = ap.parse_args()
    load_library()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)
    out = {}
    with torch.cuda.stream(side):
        out["config4_H8"] = config4(args, dev, side)
        torch.cuda.empty_cache()
        out["wide_16x128_on_4"] = wide(args, dev, side)
    torch.cuda.empty_cache()
    if not args.no_engine:
        out["engine_16x128_on_4"] = {k: engine_wide(k) for k in ("PAGED_BF16", "PAGED_FP8")}
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
