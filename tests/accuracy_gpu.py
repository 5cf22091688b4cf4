"""What the accuracy tests of the paged scans share on the device: the page pool of a case converted to the page
element type ON the device, the float64 model and the fp32 oracle's scan of exactly what the pages hold, the lean scan
launched once or twice, and the Checker that prints and records every figure before anything is asserted.  Used by
tests/test_attention_accuracy_gpu.py and tests/test_stream_partition_gpu.py."""
from types import SimpleNamespace

import numpy as np
import torch

import f64_model as fm
from accuracy_cases import apply_family, fill_pages, oracle_scan
from gpu_util import host
from helpers import PAGE, assert_equal

SENTINEL = 12345.0
ELEM = {"f32": 0, "bf16": 1, "fp8": 2}
ESIZE = {"f32": 4, "bf16": 2, "fp8": 1}
REPORT = {}


def to_device(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


class Checker:
    """Collects the comparisons of one test: every figure is printed and recorded before anything is asserted."""

    def __init__(self, family, elem="f32"):
        self.family, self.elem, self.failures = family, elem, []

    def check(self, path, what, err_rows, e_oracle_rows):
        tol = fm.tolerance(e_oracle_rows)
        worst = float(np.max(err_rows)) if len(err_rows) else 0.0
        e_or = float(np.max(e_oracle_rows)) if len(e_oracle_rows) else 0.0
        print(f"ACCURACY {path} | {self.elem} | {self.family} | {what}: kernel {worst:.3e}  oracle {e_or:.3e}  tol {tol:.3e}")
        rec = REPORT.setdefault((path, self.elem, self.family, what), {"kernel": 0.0, "oracle": 0.0, "ratio": 0.0, "cases": 0})
        rec["kernel"] = max(rec["kernel"], worst) if np.isfinite(worst) else float("inf")
        rec["oracle"] = max(rec["oracle"], e_or)
        rec["ratio"] = max(rec["ratio"], worst / tol)
        rec["cases"] += 1
        if not worst <= tol:
            bad = np.nonzero(~(np.asarray(err_rows) <= tol))[0]
            self.failures.append(f"{path} [{self.elem}, {self.family}] {what}: {worst:.3e} > tol {tol:.3e} "
                                 f"(oracle {e_or:.3e}) in rows {bad[:8].tolist()}")

    def done(self):
        assert not self.failures, "\n".join(self.failures)


def pages_on_device(oracle, dev, c, q, kt, v, elem, poison):
    """(device pool in the page element type, float32 values the pages hold).  The fp32 pool is converted ON THE DEVICE --
    torch's round-to-nearest-even cast for bf16, the library's own mli_f32_to_fp8 for fp8, both checked against the numpy
    definitions elsewhere in the suite -- and read back, so the model sees exactly what the kernels will read."""
    from helpers import fp8_decode
    from min_llm_inference_amd import ops
    pool32, off = fill_pages(oracle, c, q, kt, v, finite_poison=poison == "finite")
    t = to_device(pool32, dev)
    offs = to_device(off, dev) if poison == "nan" and len(off) else None
    if elem == "f32":
        pool, values = t, pool32                     # (the model never reads a dead slot)
        if offs is not None:
            pool[offs] = float("nan")
    elif elem == "bf16":
        pool = t.to(torch.bfloat16)
        values = pool.float().cpu().numpy()
        if offs is not None:
            pool.view(torch.int16)[offs] = 0x7FC0
    else:
        assert poison == "nan"
        pool = ops.f32_to_fp8(t)
        lut = to_device(fp8_decode(np.arange(256, dtype=np.uint8)), dev)
        values = lut[pool.long()].cpu().numpy()
        if offs is not None:
            pool[offs] = 0x7f
    return pool, values


def paged_inputs(oracle, dev, c, family, elem, poison="nan", n_sequence=None):
    """Pages of the family on the device, the float64 model of what they hold, and the oracle's scan of the same.
    n_sequence: what the kernels are told when the case's caches are shorter (stream_model.vector_case): the page table
    is widened to n_sequence / 16 entries per row, the new ones null."""
    q, kt = apply_family(c, family)
    B, D, S = kt.shape
    L = c["lengths"]
    pool, values = pages_on_device(oracle, dev, c, q, kt, c["v_cache"], elem, poison)
    s_live = max(-(-int(L.max()) // 16) * 16, 16)          # the model and the oracle never look beyond the longest row
    k_rows = fm.gather_pages(values, c["table"], L, s_live, D, 1)
    v_rows = fm.gather_pages(values, c["table"], L, s_live, D, 2)
    ktm = k_rows.transpose(0, 2, 1)
    model = fm.Model(q, ktm, v_rows, L)
    table = np.where(c["table"] >= 0, pool.data_ptr() + ESIZE[elem] * c["table"], 0).astype(np.int64)
    if n_sequence is not None and n_sequence != S:
        assert n_sequence > S and n_sequence % PAGE == 0
        table = np.concatenate([table, np.zeros((B, (n_sequence - S) // PAGE), np.int64)], axis=1)
        S = n_sequence
    table = to_device(table, dev)
    return SimpleNamespace(q=to_device(q, dev), L=to_device(L, dev), page_table=table, pool=pool, model=model, B=B, S=S, D=D,
                           oracle=oracle_scan(oracle, q, ktm, v_rows, L), lengths=L, k_rows=k_rows, v_rows=v_rows, q_host=q)


def elems_for(D):
    from min_llm_inference_amd import ops
    out = ["f32"]
    if D % 8 == 0:
        out.append("bf16")
    if D % 16 == 0 and ops.has_fp8():
        out.append("fp8")
    return out


def lean(ops, x, elem, out=None):
    out = torch.full((x.B, x.D), SENTINEL, device=x.q.device) if out is None else out.fill_(SENTINEL)
    ops.decode_scan_paged(x.q, x.page_table, x.L, None, out, ELEM[elem], phases=7, n_sequence=x.S)
    return host(out).copy()


def lean_twice(ops, x, elem, what):
    """Two launches: the second finds the arrival counters back at zero, and gives the same bits."""
    a = lean(ops, x, elem)
    b = lean(ops, x, elem)
    assert_equal(b, a, what=f"{what}: second launch")
    return a
