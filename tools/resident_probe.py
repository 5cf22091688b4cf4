"""The resident slice of the equal-shares scan (mli_tune "scan_resident_mib"): the lean scan alone at
config 4 for bf16 / f32 / fp8 pages, swept over the MiB kept under the default cache policy.  Two forms per value: `reuse` =
back-to-back launches over one workload, as decode re-reads its pages step after step; `control` = launches alternating
between two independently allocated workloads, the same policy mix with nothing re-read.  HIP events around `--launches`
launches per point, `--rounds` rounds in alternating order.  Appends a run to profiles/resident_probe.json."""
import argparse, datetime, json, os, socket, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import bench
from min_llm_inference_amd import load_library, ops
from step_probe import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtypes", default="bf16,f32,fp8")
    ap.add_argument("--values", default="0,64,128,160,192,224")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resident_probe.json"))
    a = ap.parse_args()
    lib = load_library()
    dev = torch.device("cuda:0"); torch.cuda.set_device(dev)
    side = torch.cuda.Stream(device=dev)
    values = [int(v) for v in a.values.split(",")]
    if lib.mli_tune(b"scan_resident_mib", values[0]) != 0:   # a library from before the key: the one point it has
        values = [0]
    run = {"box": socket.gethostname(), "date": datetime.date.today().isoformat(), "label": a.label,
           "launches_per_point": a.launches, "rounds": a.rounds, "us_per_launch": {}}
    with torch.cuda.stream(side):
        for dt in a.dtypes.split(","):
            if dt == "fp8" and not ops.has_fp8():
                continue
            wls = [bench.Workload("c4", dev, seed, headroom=8, dtype=dt) for seed in (0x5EED, 0x5EED + 1)]
            def scan(wl):
                ops.decode_scan_paged(wl.q_output, wl.page_table, wl.lengths, None, wl.attention_result, wl.elem, phases=7, n_sequence=wl.S)
            state = {"i": 0}
            def alternate():
                state["i"] ^= 1
                scan(wls[state["i"]])
            mb = [wl.algorithmic_bytes(wl.lengths_host)["scan_lean"] / 1e6 for wl in wls]
            rec = {"scan_MB": [round(m, 1) for m in mb], "reuse": {str(v): [] for v in values}, "control": {str(v): [] for v in values}}
            for r in range(a.rounds):
                for v in (values if r % 2 == 0 else values[::-1]):
                    if len(values) > 1:
                        lib.mli_tune(b"scan_resident_mib", v)
                    rec["reuse"][str(v)].append(round(timed(lambda: scan(wls[0]), a.launches, side), 1))
                    rec["control"][str(v)].append(round(timed(alternate, a.launches, side), 1))
            run["us_per_launch"][dt] = rec
            for form in ("reuse", "control"):
                for v in values:
                    us = sorted(rec[form][str(v)])[len(rec[form][str(v)]) // 2]
                    print(f"{a.label} {dt} {form:7s} R {v:3d} MiB: {rec[form][str(v)]} us, median {mb[0] / us:.3f} TB/s", flush=True)
            del wls; torch.cuda.empty_cache()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.setdefault("scan_runs", []).append(run)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
