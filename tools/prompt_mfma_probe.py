"""The prompt scan on matrix instructions (mli_prompt_scan_paged_mfma) timed on an MI355X against the lane-group
prompt scan (mli_prompt_scan_paged) at tools/prompt_scan_probe.py's shape, and alone at a width only it takes.

  shared   64 rows of 1023 prompt tokens (n_sequence 1024), emb_dim 512, bf16 pages, 8 heads and 8 heads on 2 K/V heads: the two
           kernels on the same pages, q and segments, alternating region by region in one process; HIP events on the launch
           stream; median / min / max of the regions' time
  wide     the same rows at emb_dim 4096, 32 heads of 128 on 8 K/V heads: no comparison partner
  Reported per kernel: queries per workgroup, us, the K/V bytes requested (every block of TQ queries its attended prefix once
  per K/V head), and for the MFMA kernel the bf16 matrix flop it issues (3 parts x (K . q + P . V) per visited page and column
  tile: 12 * 16 * 16 * head_dim) as a rate beside the dense bf16 peak.

  python tools/prompt_mfma_probe.py [--out profiles/prompt_mfma_probe.json] [--regions 5]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from min_llm_inference_amd import load_library, ops  # noqa: E402
from tools.prompt_scan_probe import stats, timed  # noqa: E402

HBM_PEAK, MFMA_BF16_PEAK = 8.0e12, 2516.6e12   # MI355X spec: bytes/s, dense bf16 flop/s
B, S, L, BF16 = 64, 1024, 1023, 1


def block_pages(tq):
    """pages the blocks of one segment of L queries from position 0 visit, summed"""
    return sum((min((j + 1) * tq, L) - 1) // 16 + 1 for j in range(-(-L // tq)))


def case(D, H, Hkv, shared, regions, dev):
    g = torch.Generator(device=dev)
    g.manual_seed(17 + H + Hkv)
    n_pages = B * S // 16
    pool = ((torch.rand(n_pages * 16 * 3 * D, device=dev, generator=g) * 2 - 1) / 8).to(torch.bfloat16)
    order = torch.randperm(n_pages, generator=torch.Generator().manual_seed(3)).to(torch.int64)
    table = (pool.data_ptr() + order * 16 * 3 * D * 2).reshape(B, S // 16).to(dev)
    n_q = B * L
    q = torch.rand(n_q, D, device=dev, generator=g) * 2 - 1
    out, ref = torch.empty(n_q, D, device=dev), torch.empty(n_q, D, device=dev)
    arrays, max_count, _ = ops._segments([(b, 0, L) for b in range(B)], dev)
    seg_arrays = (*arrays, max_count)
    hd, grp = D // H, H // Hkv
    tq = {"mfma": ops.prompt_scan_mfma_tq(D, H, Hkv)}
    runs = {"mfma": lambda: ops.prompt_scan_paged(q, table, None, out, B, S, BF16, n_heads=H, n_kv_heads=Hkv,
                                                  seg_arrays=seg_arrays, mfma=True)}
    if shared:
        tq["lane_group"] = ops.prompt_scan_tq(D, H, BF16)
        runs["lane_group"] = lambda: ops.prompt_scan_paged(q, table, None, ref, B, S, BF16, n_heads=H, n_kv_heads=Hkv,
                                                           seg_arrays=seg_arrays)
    stream = torch.cuda.current_stream()
    for fn in runs.values():
        fn()
    stream.synchronize()
    times = {k: [] for k in runs}
    for _ in range(regions):
        for k, fn in runs.items():
            times[k].append(timed(fn, stream))
    rec = {"emb_dim": D, "n_heads": H, "n_kv_heads": Hkv, "queries": n_q}
    if shared:
        rec["max_abs_difference"] = float((out - ref).abs().max())
    for k in runs:
        r = dict(stats(times[k]), tq=tq[k])
        t = r["median_us"] * 1e-6
        # the lane-group kernel loads a K/V head once per query head of a block, the MFMA kernel once per K/V head
        width = Hkv * hd if k == "mfma" else D
        r["kv_bytes"] = B * block_pages(tq[k]) * 16 * 2 * width * 2
        r["bytes_per_s"] = r["kv_bytes"] / t
        r["share_of_hbm_peak"] = r["bytes_per_s"] / HBM_PEAK
        if k == "mfma":
            tiles = tq[k] * grp // 16
            r["mfma_flop"] = B * Hkv * block_pages(tq[k]) * tiles * 12 * 16 * 16 * hd
            r["mfma_flop_per_s"] = r["mfma_flop"] / t
            r["share_of_bf16_mfma_peak"] = r["mfma_flop_per_s"] / MFMA_BF16_PEAK
        rec[k] = r
    if shared:
        rec["lane_group_over_mfma"] = rec["lane_group"]["median_us"] / rec["mfma"]["median_us"]
    print(json.dumps(rec))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_mfma_probe.json"))
    ap.add_argument("--regions", type=int, default=5)
    args = ap.parse_args()
    load_library()
    dev = torch.device("cuda:0")
    report = {"shape": {"rows": B, "prompt_tokens": L, "n_sequence": S, "elem": "bf16"}, "hbm_peak_bytes_per_s": HBM_PEAK,
              "bf16_mfma_peak_flop_per_s": MFMA_BF16_PEAK, "cases": []}
    for D, H, Hkv, shared in ((512, 8, 8, True), (512, 8, 2, True), (4096, 32, 8, False)):
        report["cases"].append(case(D, H, Hkv, shared, args.regions, dev))
        torch.cuda.empty_cache()
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
