"""What the causal multi-query scan saves against the only way the parent could compute prompt attention: the decode scan run
over "virtual rows" (virtual row (b, t) = row b's pages with length t + 1), which reads O(L^2) K/V bytes per prompt.

  scan     64 rows of 1023 prompt tokens (n_sequence 1024), emb_dim 512, bf16 and fp32 pages, one head and 8 heads:
           mli_prompt_scan_paged (one launch, one segment per row) against mli_decode_scan_paged_gqa over the same 65472 queries
           as virtual rows (launches of at most 16384 rows: the arrival counters' limit), same pages, same q, same process.
           The two alternate region by region; HIP events on the launch stream; median / min / max of the regions' time.
           Reported per variant: TQ, us, the K/V bytes the kernel requests (the decode form: every query its whole prefix;
           the prompt form: every block of TQ queries the block's prefix once), achieved bytes/s and flop/s (4 flop per
           attended (query, slot, column): q.K and p.V) beside the HBM peak and the fp32 VALU peak, and the gain.
  engine   (--engine) bench.py's engine workload at emb_dim 512, PAGED_GEMM with logprobs, without and with prompt_logprobs,
           alternating: tokens/s

  python tools/prompt_scan_probe.py [--out profiles/prompt_scan_probe.json] [--regions 5] [--engine]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from min_llm_inference_amd import load_library, ops  # noqa: E402

HBM_PEAK, VALU_FP32_PEAK = 8.0e12, 157.3e12   # MI355X spec: bytes/s, flop/s
B, S, D, L = 64, 1024, 512, 1023
MAX_ROWS = 16384


def timed(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    stream.synchronize()
    return e0.elapsed_time(e1) * 1e3  # us


def stats(v):
    v = sorted(v)
    return {"median_us": v[len(v) // 2], "min_us": v[0], "max_us": v[-1], "regions": len(v)}


def scan_case(elem_name, H, regions, dev):
    elem = {"f32": 0, "bf16": 1}[elem_name]
    dtype = torch.float32 if elem == 0 else torch.bfloat16
    esize = 4 if elem == 0 else 2
    g = torch.Generator(device=dev)
    g.manual_seed(11 + H)
    n_pages = B * S // 16
    pool = ((torch.rand(n_pages * 16 * 3 * D, device=dev, generator=g) * 2 - 1) / 8).to(dtype)
    order = torch.randperm(n_pages, generator=torch.Generator().manual_seed(3)).numpy().astype(np.int64)
    table = torch.from_numpy((pool.data_ptr() + order * 16 * 3 * D * esize).reshape(B, S // 16)).to(dev)
    n_q = B * L
    q = torch.rand(n_q, D, device=dev, generator=g) * 2 - 1
    out = torch.empty(n_q, D, device=dev)
    ref = torch.empty(n_q, D, device=dev)
    segments = [(b, 0, L) for b in range(B)]
    rows = np.repeat(np.arange(B), L)
    pos = np.tile(np.arange(L), B)
    v_table = table[torch.from_numpy(rows).to(dev)].contiguous()
    v_len = torch.from_numpy((pos + 1).astype(np.int32)).to(dev)
    tq = ops.prompt_scan_tq(D, H, elem)
    arrays, max_count, _ = ops._segments(segments, dev)
    seg_arrays = (*arrays, max_count)

    def prompt():
        ops.prompt_scan_paged(q, table, None, out, B, S, elem, n_heads=H, seg_arrays=seg_arrays)

    def decode():
        for a in range(0, n_q, MAX_ROWS):
            b = min(a + MAX_ROWS, n_q)
            ops.decode_scan_paged_gqa(q[a:b], v_table[a:b], v_len[a:b], ref[a:b], H, H, 0, 0, elem, S)

    stream = torch.cuda.current_stream()
    ops.workspace_for(MAX_ROWS, S, D, dev, H)        # grown once, before anything is timed
    prompt(), decode()
    stream.synchronize()
    diff = float((out - ref).abs().max())
    t_prompt, t_decode = [], []
    for _ in range(regions):
        t_prompt.append(timed(prompt, stream))
        t_decode.append(timed(decode, stream))
    kv = 2 * D * esize                                                       # K and V bytes of one slot
    slots = B * L * (L + 1) // 2                                             # attended (query, slot) pairs
    bytes_decode = slots * kv
    blocks = -(-L // tq)
    bytes_prompt = B * sum(min((j + 1) * tq, L) for j in range(blocks)) * kv
    flop = 4 * slots * D
    rec = {"elem": elem_name, "n_heads": H, "tq": tq, "queries": n_q, "max_abs_difference": diff, "flop": flop,
           "prompt_scan": dict(stats(t_prompt), kv_bytes=bytes_prompt), "decode_scan_virtual_rows": dict(stats(t_decode), kv_bytes=bytes_decode)}
    for k in ("prompt_scan", "decode_scan_virtual_rows"):
        t = rec[k]["median_us"] * 1e-6
        rec[k]["bytes_per_s"] = rec[k]["kv_bytes"] / t
        rec[k]["flop_per_s"] = flop / t
        rec[k]["share_of_hbm_peak"] = rec[k]["bytes_per_s"] / HBM_PEAK
        rec[k]["share_of_valu_fp32_peak"] = rec[k]["flop_per_s"] / VALU_FP32_PEAK
    rec["gain"] = rec["decode_scan_virtual_rows"]["median_us"] / rec["prompt_scan"]["median_us"]
    print(f"{elem_name} H{H} TQ{tq}: prompt scan {rec['prompt_scan']['median_us']:.0f} us, decode scan over virtual rows "
          f"{rec['decode_scan_virtual_rows']['median_us']:.0f} us, gain {rec['gain']:.2f}x, "
          f"{rec['prompt_scan']['flop_per_s'] / 1e12:.1f} Tflop/s, max |difference| {diff:.2e}")
    return rec


def engine_case(regions, dev):
    """bench.py's engine workload (e1: 1024 slots, n_sequence 128, 2048 items with prompts of 1 .. 64 tokens, half the
    worst-case pool) at emb_dim 512 -- e1's own 2048 is beyond the prompt scan's rows -- PAGED_GEMM with logprobs (n_top 0),
    without and with prompt_logprobs, alternating: tokens/s."""
    from min_llm_inference_amd import engine as eng
    Be, Se, De, V = 1024, 128, 512, 1024
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    weights = (u(V, De), u(Se, De), u(De, De, scale=1 / np.sqrt(De)), u(De, De, scale=1 / np.sqrt(De)), u(De, De, scale=1 / np.sqrt(De)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(2 * Be)]
    rates = {False: [], True: []}
    for _ in range(regions):
        for prompt in (False, True):
            e = eng.Engine(eng.PAGED_GEMM, Be, Se, De, V, *weights, n_blocks=Be * Se // 32, logprobs=0, prompt_logprobs=prompt)
            try:
                for i, toks in items:
                    e.add_item(i, toks)
                st = e.run()
                rates[prompt].append(st.total_tokens / st.seconds)
                if prompt:
                    scored = sum(len(v[0]) for v in e.finished_prompt_logprobs().values())
            finally:
                e.close()
    rec = {"shape": {"kind": "PAGED_GEMM", "n_batch": Be, "n_sequence": Se, "emb_dim": De, "n_vocab": V, "items": len(items)},
           "prompt_positions_scored": scored}
    for prompt, key in ((False, "without_prompt_logprobs"), (True, "with_prompt_logprobs")):
        v = sorted(rates[prompt])
        rec[key] = {"median_tokens_per_s": v[len(v) // 2], "min": v[0], "max": v[-1], "runs": len(v)}
    print(f"engine: {rec['without_prompt_logprobs']['median_tokens_per_s']:.0f} tokens/s without, "
          f"{rec['with_prompt_logprobs']['median_tokens_per_s']:.0f} with prompt_logprobs ({scored} prompt positions scored)")
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prompt_scan_probe.json"))
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--engine", action="store_true", help="also the engine with and without prompt_logprobs")
    args = ap.parse_args()
    load_library()
    dev = torch.device("cuda:0")
    report = {"shape": {"rows": B, "prompt_tokens": L, "n_sequence": S, "emb_dim": D}, "hbm_peak_bytes_per_s": HBM_PEAK,
              "valu_fp32_peak_flop_per_s": VALU_FP32_PEAK, "scan": []}
    for elem_name in ("bf16", "f32"):
        for H in (1, 8):
            report["scan"].append(scan_case(elem_name, H, args.regions, dev))
            torch.cuda.empty_cache()
    if args.engine:
        report["engine"] = engine_case(args.regions, dev)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
