"""What a plain `bench.py` run does and what `--dump-outputs DIR` writes.  CPU: the dump of a small hand-built state
(page slots and contiguous caches gathered at the right positions, dtypes, names).  GPU: a plain run times exactly
--steps steps in one region, carries none of the --full blocks, and two runs with the same arguments dump the same
outputs."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
PAGE = 16


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def _state(layout, pool_dtype=torch.float32, B=5, D=8, S=64, seed=3):
    """A CPU stand-in for bench.Workload after a few steps: every tensor dump_outputs reads."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.default_rng(seed)
    lengths = torch.from_numpy(rng.integers(2, S - 1, size=B).astype(np.int32))
    wl = types.SimpleNamespace(layout=layout, B=B, D=D, S=S, dev=torch.device("cpu"), lengths=lengths,
                               q_output=torch.rand(B, D, generator=g), attention_result=torch.rand(B, D, generator=g),
                               qkt_output=torch.rand(B, S, generator=g), emb_score=torch.rand(B, 32, generator=g),
                               decoder_result=torch.from_numpy(rng.integers(0, 1000, size=(B, 1)).astype(np.int32)))
    if layout == "paged":
        W = S // PAGE
        n_pages = B * W
        raw = torch.randint(0, 120, (n_pages * PAGE * 3 * D,), generator=g, dtype=torch.uint8)
        wl.pool = raw if pool_dtype == torch.uint8 else (torch.rand(raw.shape, generator=g) * 2 - 1).to(pool_dtype)
        wl.page_ids = rng.permutation(n_pages).reshape(B, W).astype(np.int64)
    else:
        wl.inp_embedding = torch.rand(B, S, D, generator=g)
        wl.kt_cache = torch.rand(B, D, S, generator=g)
        wl.v_cache = torch.rand(B, S, D, generator=g)
    return wl


def _expected_slots(wl):
    """K, V at slot length-2 and x at slot length-1 of every row, read element by element."""
    L = wl.lengths.numpy()
    kv = np.zeros((wl.B, 2, wl.D), np.float32)
    x = np.zeros((wl.B, wl.D), np.float32)
    if wl.layout == "paged":
        pool = wl.pool.view(torch.float8_e4m3fn) if wl.pool.dtype == torch.uint8 else wl.pool
        pool = pool.float().numpy()

        def elem(b, s, seg):
            base = (wl.page_ids[b, s // PAGE] * PAGE + s % PAGE) * 3 * wl.D + seg * wl.D
            return pool[base:base + wl.D]
        for b in range(wl.B):
            kv[b, 0], kv[b, 1], x[b] = elem(b, L[b] - 2, 1), elem(b, L[b] - 2, 2), elem(b, L[b] - 1, 0)
    else:
        for b in range(wl.B):
            kv[b, 0] = wl.kt_cache[b, :, L[b] - 2].numpy()
            kv[b, 1] = wl.v_cache[b, L[b] - 2].numpy()
            x[b] = wl.inp_embedding[b, L[b] - 1].numpy()
    return kv, x


@pytest.mark.parametrize("layout,pool_dtype", [("paged", torch.float32), ("paged", torch.bfloat16),
                                               ("paged", torch.uint8), ("naive", None)])
@pytest.mark.parametrize("materialising", [False, True])
def test_dump_outputs_writes_the_step_results_and_the_written_slots(tmp_path, layout, pool_dtype, materialising):
    bench = _bench()
    wl = _state(layout, pool_dtype)
    bench.dump_outputs(wl, str(tmp_path), materialising=materialising)
    names = {"q_output", "attention_result", "tokens", "lengths", "sample_rows", "sample_new_kv", "sample_new_x"}
    if materialising:
        names |= {"probabilities", "emb_score"}
    assert {f[:-4] for f in os.listdir(tmp_path)} == names
    a = {n: np.load(tmp_path / f"{n}.npy") for n in names}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    np.testing.assert_array_equal(a["q_output"], wl.q_output.numpy())
    np.testing.assert_array_equal(a["attention_result"], wl.attention_result.numpy())
    np.testing.assert_array_equal(a["tokens"], wl.decoder_result.numpy().reshape(-1))
    np.testing.assert_array_equal(a["lengths"], wl.lengths.numpy())
    rows = a["sample_rows"].astype(np.int64)
    np.testing.assert_array_equal(rows, np.arange(wl.B))      # B < the sample size: every row, in order
    kv, x = _expected_slots(wl)
    np.testing.assert_array_equal(a["sample_new_kv"], kv[rows])
    np.testing.assert_array_equal(a["sample_new_x"], x[rows])
    if materialising:
        np.testing.assert_array_equal(a["probabilities"], wl.qkt_output.numpy())
        np.testing.assert_array_equal(a["emb_score"], wl.emb_score.numpy())


def test_dump_sample_of_a_large_batch_is_fixed_and_bounded(tmp_path):
    bench = _bench()
    wl = _state("paged", B=600, D=8, S=64)
    bench.dump_outputs(wl, str(tmp_path / "a"), materialising=False)
    bench.dump_outputs(wl, str(tmp_path / "b"), materialising=False)
    ra, rb = (np.load(tmp_path / d / "sample_rows.npy") for d in ("a", "b"))
    assert len(ra) == bench.DUMP_SAMPLE_ROWS and (np.diff(ra) > 0).all()
    np.testing.assert_array_equal(ra, rb)
    kv, x = _expected_slots(wl)
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "sample_new_kv.npy"), kv[ra.astype(np.int64)])


def _plain_run(args, timeout=600):
    r = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_exactly_steps_and_dumps_the_same_outputs_twice(tmp_path):
    common = ["--gpus", "1", "--workload", "c3", "--steps", "7", "--warmup", "2"]
    first = _plain_run(common + ["--dump-outputs", str(tmp_path / "a")])
    second = _plain_run(common + ["--dump-outputs", str(tmp_path / "b")])
    for out in (first, second):
        assert out["steps"] == 7 and out["warmup"] == 2 and out["repeat"]["regions"] == 1
        assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(256 * 1e3 / out["ms_per_step"], rel=1e-9)
        assert not {"roofline", "modes", "configs", "cpu_baseline", "collective"} & set(out)
    a = {f: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    b = {f: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert set(a) == set(b) and "attention_result.npy" in a and "tokens.npy" in a
    lengths0 = a["lengths.npy"] - 7                          # every row grew by exactly the timed steps
    assert (lengths0 >= 1024 // 4).all()
    np.testing.assert_array_equal(a["tokens.npy"], b["tokens.npy"])
    np.testing.assert_array_equal(a["lengths.npy"], b["lengths.npy"])
    for f in a:
        np.testing.assert_allclose(a[f], b[f], rtol=1e-5, atol=1e-6, err_msg=f)
