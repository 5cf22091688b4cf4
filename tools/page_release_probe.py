"""What early page release (mli_engine_set_page_release) and the windowed prefill (mli_paged_prefill_window) cost and gain,
against the same runs without them and, where a second source tree is given, against that tree's library (the parent
commit's, built beside this one) on the same box.

  price     PAGED_BF16 engine at the window_probe setting -- B 1024, S 4096, D 512, 2048 items with prompts of 1 .. 64, pool =
            half the worst case, W 1024 -- with K = 0 and K = 4: release off (other tree / this tree) and release on.
            tokens/s, iterations, preemptions, peak pages in use.
  capacity  the same pool with n_batch raised to the largest value with n_batch x (per-row bound) <= pool, 2 n_batch items,
            release on.
  prefill   bf16, D 512, S 4096, 64 new rows: mli_paged_prefill (other tree / this tree) against mli_paged_prefill_window at
            W 1024, K 4, on rows of L = 4095 (live share (16 + 1024 + 15) / 4095) and on rows of L <= W (all live).  HIP
            events, regions of 10 launches after a warm-up.

Every measurement is a process of its own (one GPU process at a time); the variants alternate round by round, so a drift of
the box lands on all of them.  median / min / max over the rounds.

  python tools/page_release_probe.py [--other-root DIR] [--rounds 3] [--out profiles/page_release_probe.json] [--skip ...]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, S, D, W = 1024, 4096, 512, 1024
POOL = B * S // 32


def bound(ahead, sinks):
    return -(-sinks // 16) + -(-(W + ahead) // 16) + 1


# ---- workers (fresh processes; `root` chooses the tree whose package and library are loaded) -----------------------------
def _import(root):
    sys.path.insert(0, root)
    import bench
    from min_llm_inference_amd import engine as eng, load_library, ops
    return bench, eng, load_library(), ops


def work_engine(root, n_batch, n_items, sinks, release):
    import numpy as np
    bench, eng, _, ops = _import(root)
    V = bench.N_VOCAB
    rng = np.random.default_rng(0x5EED0100)

    def u(*shape, scale=1.0):
        return ((rng.random(shape, dtype=np.float32) * 2 - 1) * np.float32(scale)).astype(np.float32)

    emb = u(V, D)
    emb[ops.EOF_TOKEN_ID] *= 1.0001
    weights = (emb, u(S, D), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)), u(D, D, scale=1 / np.sqrt(D)))
    items = [(i, rng.integers(0, ops.EOF_TOKEN_ID, size=int(rng.integers(1, 65)))) for i in range(n_items)]
    kw = dict(release_pages=True) if release else {}
    e = eng.Engine(eng.PAGED_BF16, n_batch, S, D, V, *weights, n_blocks=POOL, window=W, sinks=sinks or None, **kw)
    for i, toks in items:
        e.add_item(i, toks)
    st = e.run()
    out = {"tokens": int(st.total_tokens), "seconds": round(st.seconds, 3), "iterations": int(st.iterations),
           "tokens_per_s": round(st.total_tokens / st.seconds, 1)}
    if hasattr(e, "page_stats"):
        p = e.page_stats()
        out.update(preemptions=int(p.preemptions), peak_pages_in_use=int(p.peak_in_use), released_early=int(p.released_early))
    e.close()
    assert st.finished == n_items
    return out


REGION_MS = 100.0


def work_prefill(root, sinks, regions):
    import numpy as np
    import torch
    _, _, _, ops = _import(root)
    dev = torch.device("cuda:0")
    n_new, V = 64, 1024
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    rand = lambda *shape: torch.rand(*shape, device=dev, generator=g) * 2 - 1
    emb, wpe = rand(V, D), rand(S, D)
    wk, wv = (rand(D, D) / D ** 0.5).to(torch.bfloat16), (rand(D, D) / D ** 0.5).to(torch.bfloat16)
    inp = torch.randint(0, V, (n_new, S), device=dev, generator=g, dtype=torch.int32)
    page = 16 * 3 * D
    pool = torch.zeros(n_new * (S // 16) * page, dtype=torch.bfloat16, device=dev)
    table = (pool.data_ptr() + 2 * page * torch.arange(n_new * (S // 16), device=dev, dtype=torch.int64)).reshape(n_new, S // 16)
    idx = torch.arange(n_new, device=dev, dtype=torch.int32)
    rng = np.random.default_rng(5)
    lengths = {"L4095": torch.full((n_new,), S - 1, device=dev, dtype=torch.int32),
               "L_le_W": torch.from_numpy(rng.integers(1, W + 1, size=n_new).astype(np.int32)).to(dev)}
    has_window = "window" in ops.paged_prefill.__code__.co_varnames
    variants = {}
    for name, L in lengths.items():
        variants[f"{name}_plain"] = lambda L=L: ops.paged_prefill(emb, wpe, inp, table, L, idx, wk, wv, n_new)
        if has_window:
            variants[f"{name}_window"] = lambda L=L: ops.paged_prefill(emb, wpe, inp, table, L, idx, wk, wv, n_new, window=W, sinks=sinks)
    stream = torch.cuda.current_stream()

    def region(fn, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(launches):
            fn()
        e1.record(stream)
        stream.synchronize()
        return e0.elapsed_time(e1) / launches * 1e3

    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    launches = {k: max(10, int(REGION_MS * 1e3 / region(fn, 10))) for k, fn in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(regions):
        for k, fn in variants.items():
            times[k].append(round(region(fn, launches[k]), 1))
    return {"us_per_launch": times, "launches_per_region": launches, "live_share_L4095": round((16 * -(-sinks // 16) + W + 15) / (S - 1), 4)}


# ---- driver -------------------------------------------------------------------------------------------------------------
def spawn(*args):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", json.dumps(args)], capture_output=True, text=True,
                       timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"worker {args} failed ({r.returncode}): {r.stdout[-2000:]}{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def summary(values):
    v = sorted(values)
    return {"median": v[len(v) // 2] if len(v) % 2 else round((v[len(v) // 2 - 1] + v[len(v) // 2]) / 2, 1), "min": v[0],
            "max": v[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None)
    ap.add_argument("--other-root", default=None, help="a second source tree with its library built (the parent commit)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip", default="", help="comma list of price, capacity, prefill")
    args = ap.parse_args()
    if args.worker:
        what, *rest = json.loads(args.worker)
        print(json.dumps({"engine": work_engine, "prefill": work_prefill}[what](*rest)))
        return
    skip = set(filter(None, args.skip.split(",")))
    trees = {"this": ROOT}
    if args.other_root:
        trees = {"other": os.path.abspath(args.other_root), "this": ROOT}
    out = {"setting": {"kind": "PAGED_BF16", "n_batch": B, "n_sequence": S, "emb_dim": D, "window": W, "pool_pages": POOL,
                       "rounds": args.rounds, "trees": sorted(trees)}}

    def collect(runs):
        table = {}
        for name, rows in runs.items():
            table[name] = {"tokens_per_s": summary([r["tokens_per_s"] for r in rows]), "runs": rows}
        return table

    if "price" not in skip:
        for sinks in (0, 4):
            runs = {}
            for _ in range(args.rounds):
                for tree, root in trees.items():
                    runs.setdefault(f"{tree}_release_off", []).append(spawn("engine", root, B, 2 * B, sinks, False))
                runs.setdefault("this_release_on", []).append(spawn("engine", ROOT, B, 2 * B, sinks, True))
            table = collect(runs)
            base = table.get("other_release_off", table["this_release_off"])["tokens_per_s"]["median"]
            for row in table.values():
                row["tokens_per_s_vs_base"] = round(row["tokens_per_s"]["median"] / base, 3)
            out[f"price_K{sinks}"] = table
            print(json.dumps({f"price_K{sinks}": {k: (v["tokens_per_s"], v["tokens_per_s_vs_base"]) for k, v in table.items()}}), flush=True)
    if "capacity" not in skip:
        for sinks in (0, 4):
            n_batch = POOL // bound(2, sinks)
            rows = [spawn("engine", ROOT, n_batch, 2 * n_batch, sinks, True) for _ in range(args.rounds)]
            out[f"capacity_K{sinks}"] = {"n_batch": n_batch, "per_row_bound": bound(2, sinks), **collect({"release_on": rows})["release_on"]}
            print(json.dumps({f"capacity_K{sinks}": {"n_batch": n_batch, "tokens_per_s": out[f"capacity_K{sinks}"]["tokens_per_s"]}}), flush=True)
    if "prefill" not in skip:
        merged = {}
        for _ in range(args.rounds):
            for tree, root in trees.items():
                r = spawn("prefill", root, 4, 5)
                out.setdefault("prefill", {})["live_share_L4095"] = r["live_share_L4095"]
                out["prefill"].setdefault("launches_per_region", {}).update({f"{tree}_{k}": n for k, n in r["launches_per_region"].items()})
                for k, t in r["us_per_launch"].items():
                    merged.setdefault(f"{tree}_{k}", []).extend(t)
        out["prefill"]["us_per_launch"] = {k: {**summary(t), "regions": t} for k, t in merged.items()}
        med = {k: v["median"] for k, v in out["prefill"]["us_per_launch"].items()}
        base = "other" if "other" in trees else "this"
        out["prefill"]["window_vs_plain"] = {name: round(med[f"this_{name}_window"] / med[f"{base}_{name}_plain"], 3)
                                             for name in ("L4095", "L_le_W")}
        print(json.dumps({"prefill": {"median_us": med, "window_vs_plain": out["prefill"]["window_vs_plain"]}}), flush=True)
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
