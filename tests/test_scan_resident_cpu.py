"""tests/cpp/scan_resident_test.cpp: the resident slice of the equal-shares scan (csrc/scan_plan.hpp: resident_threshold,
resident_keeps -- the text the kernel compiles).  The threshold at 0 MiB, at the clamp, without pages, with one, and at the
largest shape the kernel takes (2^35 bytes: no 32-bit overflow); the keep rule monotone in the threshold; the kept share
of page pools laid out as base + block * permutation for the (emb_dim, element size) pairs of
tests/test_scan_resident_gpu.py within 2 % of threshold / 65536, also per share of 256 pages.  A stand-alone program built
with g++ under ASan + UBSan, no HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_resident(tmp_path):
    assert shutil.which("g++")
    exe = str(tmp_path / "scan_resident_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "min_llm_inference_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "scan_resident_test.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failure(s)" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert "24 page pools of 60000 pages" in r.stdout
