"""The grouped-query scan on matrix instructions over fp32 pages (mli_decode_scan_paged_gqa_mfma_f32) timed on an
MI355X, by the method of tools/gqa_mfma_fp8_probe.py (alternated regions in one process, median / min / max).

  (a) config-4 shape  B = 1024, S = 4096, D = 512, 8 heads of 64, ragged lengths, fp32 pages, Hkv = 4 / 2 / 1 (g = 2 / 4 / 8):
      the lane-group scan (mli_decode_scan_paged_gqa, unchanged) | this kernel
  (b) wide shape      B = 256, S = 4096, 16 heads of 128 on 4 K/V heads (D = 2048, the widest fp32 row), lengths U[S/4, 3S/4]:
      the bf16 MFMA kernel on a bf16 pool | this kernel on the fp32 pool of the same values; K/V bytes per second of both against
      the streaming-read rate (mli_stream_read, 4 GiB of the fp32 pool per launch) of the same run
  (c) end to end      the PAGED engine at that shape with heads (gqa_mfma_fp8_probe.engine_wide's workload): generated tokens
      per second of wall time of one run, prefill included

  python tools/gqa_mfma_f32_probe.py [--out profiles/gqa_mfma_f32_probe.json] [--regions 7] [--launches 20] [--no-engine]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gqa_mfma_fp8_probe import engine_wide  # noqa: E402
from gqa_mfma_probe import stats, timed  # noqa: E402
from min_llm_inference_amd import load_library, ops  # noqa: E402


def versus(res, new, old):
    res[new][f"time_vs_{old}"] = round(res[new]["us_median"] / res[old]["us_median"], 3)
    return res


def config4(args, dev, side):
    H, out = 8, {}
    wl = bench.Workload("c4", dev, 0x5EED, headroom=8, dtype="f32")
    q = torch.rand(wl.B, wl.D, device=dev) * 2 - 1
    live = int(np.minimum(np.asarray(wl.lengths_host).astype(np.int64), wl.S).sum())
    for Hkv in (4, 2, 1):
        ops.workspace_for(wl.B, wl.S, wl.D, dev, H, mfma_kv_heads=Hkv)
        times = timed({
            "lane_group": lambda: ops.decode_scan_paged_gqa(q, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, 0, 0, ops.ELEM_F32, wl.S),
            "mfma_f32": lambda: ops.decode_scan_paged_gqa_mfma_f32(q, wl.page_table, wl.lengths, wl.attention_result, H, Hkv, 0, wl.S),
        }, args, side)
        out[f"Hkv{Hkv}"] = versus({k: stats(t, live * 2 * (wl.D // H * Hkv) * 4) for k, t in times.items()}, "mfma_f32", "lane_group")
    return {"shape": {"B": wl.B, "S": wl.S, "D": wl.D, "H": H}, "regions": args.regions, "launches_per_region": args.launches, **out}


def wide(args, dev, side):
    B, S, H, Hkv, hd = 256, 4096, 16, 4, 128
    D, W = H * hd, S // 16
    rng = np.random.default_rng(0x5EED)
    L = rng.integers(S // 4, 3 * S // 4 + 1, size=B).astype(np.int32)
    order = rng.permutation(B * W).astype(np.int64)
    pools = {"bf16": torch.empty(B * W * 16 * 3 * D, dtype=torch.bfloat16, device=dev).uniform_(-1, 1)}
    pools["f32"] = pools["bf16"].float()
    esize = {"bf16": 2, "f32": 4}
    scan = {"bf16": ops.decode_scan_paged_gqa_mfma, "f32": ops.decode_scan_paged_gqa_mfma_f32}
    tables = {dt: torch.from_numpy((p.data_ptr() + esize[dt] * 16 * 3 * D * order).reshape(B, W)).to(dev) for dt, p in pools.items()}
    q = torch.rand(B, D, device=dev) * 2 - 1
    out = torch.empty(B, D, device=dev)
    Ld = torch.from_numpy(L).to(dev)
    ops.workspace_for(B, S, D, dev, H, mfma_kv_heads=Hkv)
    n_read = 1 << 30                                    # floats: 4 GiB of the fp32 pool, far beyond the 256 MiB Infinity Cache
    stream_src, sink = pools["f32"][:n_read], torch.zeros(64, device=dev)
    variants = {dt: lambda dt=dt: scan[dt](q, tables[dt], Ld, out, H, Hkv, 0, S) for dt in scan}
    variants["stream_read"] = lambda: ops.stream_read(stream_src, sink)
    times = timed(variants, args, side)
    ceiling = stats(times["stream_read"], n_read * 4)
    res = versus({dt: stats(times[dt], int(L.astype(np.int64).sum()) * 2 * Hkv * hd * esize[dt]) for dt in scan}, "f32", "bf16")
    for dt in scan:
        res[dt]["of_stream_read_rate"] = round(res[dt]["kv_TBps"] / ceiling["kv_TBps"], 3)
    return {"shape": {"B": B, "S": S, "D": D, "H": H, "Hkv": Hkv, "lengths": "U[S/4, 3S/4]"}, **res,
            "stream_read": {"us_median": ceiling["us_median"], "MB": ceiling["kv_MB"], "TBps": ceiling["kv_TBps"]}}


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
        out["config4_H8_f32"] = config4(args, dev, side)
        torch.cuda.empty_cache()
        out["wide_16x128_on_4"] = wide(args, dev, side)
    torch.cuda.empty_cache()
    if not args.no_engine:
        out["engine_16x128_on_4"] = engine_wide("PAGED")
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
