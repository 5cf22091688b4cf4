"""tests/cpp/page_release_test.cpp: the rule for "which pages of a row are live" (csrc/page_live.hpp) against an independent
restatement from the scan's slot mask, by enumeration at n_sequence 64 and 256; and the scheduler's early page release
(PagedAttentionsManager::set_page_release) under a fake windowed model whose pages carry (item id, position) tags, in the
sequential and the pipelined loop, from roomy pools down to pools smaller than one full row.  A stand-alone program built
with g++ under ASan + UBSan over the malloc test double, no HIP.  Built with one deliberate fault in the scheduler
(-DMUTANT=1 .. 6, which the build hands to paged_item_storage.cpp as MLI_PAGE_RELEASE_MUTANT) the same program must fail."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "min_llm_inference_amd", "host")
MUTANTS = {
    1: "release by n + 1",
    2: "release of the sink pages",
    3: "release one page too far (p0 + 1)",
    4: "admission with contiguous page indices",
    5: "admission without the look-ahead",
    6: "a released page left in the row's holdings (returned twice)",
}


def _build(tmp_path, mutant):
    exe = str(tmp_path / f"page_release_test_{mutant}")
    sources = [os.path.join(ROOT, "tests", "cpp", "page_release_test.cpp"),
               os.path.join(ROOT, "tests", "cpp", "memory_host_double.cpp")]
    sources += [os.path.join(HOST, "src", f) for f in ("pipelined_engine.cpp", "item_storage.cpp", "paged_item_storage.cpp",
                                                        "throughput_counter.cpp")]
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
           "-I", os.path.join(HOST, "include"), "-I", os.path.join(ROOT, "include"), f"-DMUTANT={mutant}",
           "-DMLI_PAGE_RELEASE_MUTANT=MUTANT", "-o", exe] + sources
    return exe, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_page_release_rule_and_scheduler(tmp_path):
    assert shutil.which("g++")
    builds = {m: _build(tmp_path, m) for m in [0] + sorted(MUTANTS)}
    for m, (exe, proc) in builds.items():
        out, _ = proc.communicate()
        assert proc.returncode == 0, out[-3000:]
    r = subprocess.run([builds[0][0]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "\n0 failure(s)" in r.stdout, r.stdout[-4000:] + r.stderr[-4000:]
    assert r.stdout.count("[ OK ]") == 2 + 24 and "216 scheduler runs" in r.stdout
    # the program must bite: every mutant of the scheduler fails it (the rule part does not depend on the scheduler)
    running = {m: subprocess.Popen([builds[m][0], "scheduler"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
               for m in MUTANTS}
    for m, proc in running.items():
        out, _ = proc.communicate(timeout=600)
        assert proc.returncode != 0, f"mutant {m} ({MUTANTS[m]}) passes"
        assert "[FAIL]" in out or "Assertion" in out or "ERROR" in out, (m, out[-2000:])
