"""tests/cpp/prompt_plan_test.cpp: the host side of the prompt log-probabilities -- the pass cutting (csrc/prompt_plan.hpp: no
pass beyond n_batch positions, every position 0 .. L - 2 of every new row exactly once and in order; prompts of length 1, 2,
n_batch, n_batch + 1 and n_sequence) and the shape predicate (csrc/scan_plan.hpp: prompt_scan_shape_ok against a table).  A
stand-alone program built with g++ under ASan + UBSan the way tests/cpp/Makefile builds scan_plan_test, no HIP."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_prompt_plan(tmp_path):
    assert shutil.which("g++")
    exe = str(tmp_path / "prompt_plan_test")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(ROOT, "min_llm_inference_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "prompt_plan_test.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
