"""tests/cpp/gqa_map_test.cpp: grouped-query attention in the launch plan (csrc/scan_plan.hpp) -- the lane map gqa_kv_unit by
enumeration over every supported (elem, D, H, Hkv), gqa_shape_supported against a table of accepted and refused shapes, and
plan_chunked_scan with read width D against the plan without one, field by field.  A stand-alone program built with g++
under ASan + UBSan the way tests/cpp/Makefile builds scan_plan_test, no HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gqa_map(tmp_path):
    assert shutil.which("g++")
    exe = str(tmp_path / "gqa_map_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "min_llm_inference_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "gqa_map_test.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 failure(s)" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert "31 shape rows" in r.stdout
