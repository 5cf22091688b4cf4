"""tests/cpp/sink_plan_test.cpp: the launch plan of the paged scan with attention sinks (csrc/scan_plan.hpp: sink_span, the
hand-off rule lean_scan_kind, and the chunked plan at the sinks' span) against values worked out by hand at the shapes of
tests/test_sinks_scan_gpu.py; K = 0 gives the windowed plan and K + W >= n_sequence the plain one.  A stand-alone program
built with g++ under ASan + UBSan, no HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sink_plan(tmp_path):
    assert shutil.which("g++")
    exe = str(tmp_path / "sink_plan_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "min_llm_inference_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "sink_plan_test.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failure(s)" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert "13 sink plan rows" in r.stdout
