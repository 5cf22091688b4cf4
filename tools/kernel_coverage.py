#!/usr/bin/env python3
"""Which test files launch which kernel of the library: the record tests/kernel_coverage.json (held to the build's inventory and
to the list of judging files by tests/test_kernel_coverage_cpu.py).

    tools/kernel_coverage.py collect [--out DIR] [--files tests/test_x_gpu.py ...] [--resume] [--budget SECONDS] [--keep-traces]
    tools/kernel_coverage.py merge   [--out DIR] [--json tests/kernel_coverage.json]

collect (on the MI355X, outside pytest) runs every test file that has gpu-marked tests, one file at a time and nothing in
parallel, each as a fresh child under the profiler's kernel trace and nothing else:

    timeout -k 10 LIMIT rocprofv3 --kernel-trace --output-format csv -d DIR/<file> -- python -m pytest <file> -m gpu -q

LIMIT comes from the table below: the file's unprofiled duration times PROFILER_FACTOR, at least MIN_LIMIT.  Every exit status
is checked; after the first abnormal one (a time limit, an abort, a segmentation fault, or an illegal-memory-access message in
the output) nothing further is started and collect exits 1.  A file whose tests fail (pytest's status 1) is recorded as such and
collect goes on: its kernels were still launched; collect then exits 2.  --budget stops before a file whose limit would pass
SECONDS since the start (exit 3); --resume skips the files DIR already holds a clean run of.  After each file the distinct
Kernel_Name values of its trace are written to DIR/<file>/kernels.txt and the raw trace is removed unless --keep-traces.

merge reads those names per file (or the traces where they were kept), keeps the library's kernels (namespace mli), normalises
them as tools/kernel_inventory.py does and writes {kernel name: [test files that launched it]} -- names only, sorted, so that
the file changes only when coverage changes."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_inventory import normalise  # noqa: E402

PROFILER_FACTOR = 3.0     # measured: 1.03 over the suite, and 2 - 3 s of start-up per file; the rest is room for a slower box
MIN_LIMIT = 120           # seconds: interpreter, torch and profiler start-up dominate the short files
DEFAULT_SECONDS = 30      # a file the table does not name yet
# seconds pytest reports for `python -m pytest <file> -m gpu -q` on an MI355X, rounded up.  Taken under the kernel trace, which
# added 3 % to the suite (902 s against 874 s): an upper bound of the plain duration.
UNPROFILED_SECONDS = {
    "test_alibi_engine_gpu.py": 5, "test_alibi_scan_gpu.py": 9, "test_attention_accuracy_gpu.py": 127,
    "test_bench_launcher.py": 8, "test_bench_outputs.py": 8, "test_cpp_dropin_gpu.py": 4, "test_drawn_shapes_gpu.py": 32,
    "test_encoder_decoder_gpu.py": 3, "test_engine_dispatch_gpu.py": 23, "test_engine_gpu.py": 25,
    "test_engine_replay_gpu.py": 21, "test_full_size_properties_gpu.py": 12, "test_gemm_edges_gpu.py": 24,
    "test_golden_gpu.py": 3, "test_gqa_engine_gpu.py": 4, "test_gqa_scan_gpu.py": 12, "test_heads_engine_gpu.py": 4,
    "test_heads_instantiations_gpu.py": 4, "test_heads_scan_gpu.py": 7, "test_lean_path_gpu.py": 65,
    "test_logprobs_engine_gpu.py": 6, "test_logprobs_gpu.py": 3, "test_naive_kernels_gpu.py": 13,
    "test_page_release_engine_gpu.py": 25, "test_paged_bf16_gpu.py": 45, "test_paged_fp8_gpu.py": 77,
    "test_paged_kernels_gpu.py": 94, "test_prefill_window_gpu.py": 4, "test_prompt_logprobs_engine_gpu.py": 5,
    "test_prompt_long_gpu.py": 44, "test_prompt_scan_gpu.py": 10, "test_prompt_score_gpu.py": 3,
    "test_rope_engine_gpu.py": 6, "test_rope_gemm_gpu.py": 7, "test_rope_scan_gpu.py": 3, "test_sampling_gpu.py": 6,
    "test_scan_resident_gpu.py": 8, "test_scratch_contract_gpu.py": 8, "test_shape_limits_gpu.py": 27,
    "test_shard_group_gpu.py": 7, "test_sink_logits_engine_gpu.py": 5, "test_sink_logits_prompt_gpu.py": 4,
    "test_sink_logits_scan_gpu.py": 8, "test_sink_logits_scratch_gpu.py": 4, "test_sinks_engine_gpu.py": 5,
    "test_sinks_scan_gpu.py": 12, "test_softcap_engine_gpu.py": 5, "test_softcap_prompt_gpu.py": 5,
    "test_softcap_scan_gpu.py": 9, "test_stream_partition_gpu.py": 46, "test_window_engine_gpu.py": 5,
    "test_window_scan_gpu.py": 11,
}
ABNORMAL = {124: "time limit", 137: "killed at the time limit", 134: "abort", 139: "segmentation fault"}
FAULT_TEXT = "illegal memory access"


def gpu_test_files():
    files = []
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*.py"))):
        with open(path) as f:
            if "pytest.mark.gpu" in f.read():
                files.append(os.path.relpath(path, ROOT))
    return files


def limit_for(test_file):
    return int(max(MIN_LIMIT, PROFILER_FACTOR * UNPROFILED_SECONDS.get(os.path.basename(test_file), DEFAULT_SECONDS)))


def trace_names(directory):
    """the distinct Kernel_Name values of every kernel-trace CSV under directory"""
    names = set()
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as f:
            for row in csv.DictReader(f):
                if row.get("Kernel_Name"):
                    names.add(row["Kernel_Name"])
    return names


def in_library(name):
    return "mli::" in name


def collect(args):
    files = args.files or gpu_test_files()
    os.makedirs(args.out, exist_ok=True)
    start, failed = time.time(), []
    for test_file in files:
        stem = os.path.splitext(os.path.basename(test_file))[0]
        out = os.path.join(args.out, stem)
        status_path = os.path.join(out, "status.json")
        if args.resume and os.path.exists(status_path):
            with open(status_path) as f:
                if json.load(f).get("rc") == 0:
                    continue
        limit = limit_for(test_file)
        if args.budget and time.time() - start + limit > args.budget:
            print(f"collect: stopping before {test_file}: its limit of {limit} s would pass the budget", flush=True)
            return 3
        shutil.rmtree(out, ignore_errors=True)
        os.makedirs(out)
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "--",
               sys.executable, "-m", "pytest", test_file, "-m", "gpu", "-q"]
        t0 = time.time()
        r = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, errors="replace")
        seconds = time.time() - t0
        with open(os.path.join(out, "output.txt"), "w") as f:
            f.write(r.stdout)
        rc = r.returncode
        reason = ABNORMAL.get(rc) or (f"signal {-rc}" if rc < 0 else None) or (FAULT_TEXT if FAULT_TEXT in r.stdout else None)
        names = sorted(trace_names(out))
        with open(os.path.join(out, "kernels.txt"), "w") as f:
            f.write("".join(n + "\n" for n in names))
        if not args.keep_traces:
            for d in os.listdir(out):
                if os.path.isdir(os.path.join(out, d)):
                    shutil.rmtree(os.path.join(out, d))
        tail = [line for line in r.stdout.splitlines() if " passed" in line or " failed" in line or " error" in line][-1:]
        with open(status_path, "w") as f:
            json.dump({"file": test_file, "rc": rc, "abnormal": reason, "seconds": round(seconds, 1), "limit": limit,
                       "kernels": len(names), "summary": tail[0] if tail else ""}, f)
        print(f"collect: {test_file}: rc {rc}, {seconds:.0f} s of {limit}, {len(names)} kernel names; {tail[0] if tail else ''}",
              flush=True)
        if reason:
            print(f"collect: {test_file} ended abnormally ({reason}); nothing further is started\n" + r.stdout[-3000:], flush=True)
            return 1
        if rc != 0:
            failed.append(test_file)
            print(r.stdout[-3000:], flush=True)
    if failed:
        print("collect: tests failed in " + ", ".join(failed))
        return 2
    return 0


def merge_names(names_by_file):
    """{test file: iterable of raw kernel names} -> {normalised library kernel: sorted [test files]}"""
    record = {}
    for test_file, names in names_by_file.items():
        for name in names:
            key = normalise(name)
            if in_library(key):
                record.setdefault(key, set()).add(test_file)
    return {k: sorted(v) for k, v in sorted(record.items())}


def merge(args):
    names_by_file = {}
    for status_path in sorted(glob.glob(os.path.join(args.out, "*", "status.json"))):
        out = os.path.dirname(status_path)
        with open(status_path) as f:
            status = json.load(f)
        if status.get("abnormal"):
            sys.exit(f"merge: {status['file']} ended abnormally ({status['abnormal']}): its trace is no evidence")
        listed = os.path.join(out, "kernels.txt")
        if os.path.exists(listed):
            with open(listed) as f:
                names = {line.rstrip("\n") for line in f if line.strip()}
        else:
            names = trace_names(out)
        names_by_file[status["file"]] = names
    missing = [f for f in gpu_test_files() if f not in names_by_file]
    if missing:
        sys.exit("merge: no trace of " + ", ".join(missing))
    record = merge_names(names_by_file)
    with open(args.json, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"merge: {len(record)} kernels from {len(names_by_file)} files -> {args.json}")
    return 0


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = p.add_subparsers(dest="command", required=True)
    c = sub.add_parser("collect")
    c.add_argument("--out", default=os.path.join(ROOT, "build", "kernel_coverage"))
    c.add_argument("--files", nargs="*")
    c.add_argument("--resume", action="store_true")
    c.add_argument("--budget", type=float, default=0)
    c.add_argument("--keep-traces", action="store_true")
    m = sub.add_parser("merge")
    m.add_argument("--out", default=os.path.join(ROOT, "build", "kernel_coverage"))
    m.add_argument("--json", default=os.path.join(ROOT, "tests", "kernel_coverage.json"))
    args = p.parse_args()
    return collect(args) if args.command == "collect" else merge(args)


if __name__ == "__main__":
    sys.exit(main())
