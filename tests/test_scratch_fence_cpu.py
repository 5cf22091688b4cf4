"""The fence bites: tests/scratch_fence.py on CPU tensors, with numpy stand-ins for a kernel.  A correct
stand-in passes the whole protocol; every wrong one is rejected by the check named in its test, which is the check
tests/test_scratch_contract_gpu.py applies to the kernels.

The stand-in "kernel" is a two-chunk merge, the shape of the scans' in-launch merge: rows of a [B, 2, D] input are summed
per chunk into partial rows in the scratch body, a (weight) triple per chunk is published beside them, an arrival
counter per row and a ticket at the end of the counter region are raised and put back, and the output is the weighted
sum of the partial rows.  A row of one chunk has no second partial row: its slot in the body is stale."""
import numpy as np
import pytest
import torch

import scratch_fence as sf

B, D = 5, 8
COUNTERS = sf.COUNTER_BYTES
NEED = COUNTERS + B * 2 * 4 + B * 2 * D * 4       # counters | weights [B, 2] | partial rows [B, 2, D]
TICKET = COUNTERS // 4 - 1
SENTINEL = 12345.0


def make():
    rng = np.random.default_rng(7)
    x = rng.standard_normal((B, 2, D)).astype(np.float32)
    chunks = np.array([2, 1, 2, 0, 1], np.int32)              # rows of two chunks, one chunk and none
    a = sf.Arena(sf.Arena.room(x.nbytes, chunks.nbytes, B * D * 4, NEED, B * 2 * 4), "cpu")
    a.carve_from("x", x)
    a.carve_from("chunks", chunks)
    a.carve("out", B * D * 4)
    a.view("out", torch.float32).fill_(SENTINEL)
    a.carve("ws", NEED, "zero")
    a.carve("result", B * 2 * 4)                              # decoder_result [B, 2]: column 1 is the call's
    a.view("result", torch.int32).fill_(-7)
    return a, x, chunks


def np_view(a, name, dtype, shape, extra=0):
    """numpy view of a view's memory, `extra` bytes beyond its end included (a stand-in can overrun)."""
    start, nbytes, _ = a.views[name]
    raw = a.mem.numpy()[start:start + nbytes + extra]
    return raw if dtype is None else raw.view(dtype).reshape(shape)


def kernel(a, ws_bytes, fault=None):
    """The stand-in.  Returns the status: -12 when the scratch is too small, before anything is written (unless the fault
    says otherwise)."""
    x = np_view(a, "x", np.float32, (B, 2, D))
    chunks = np_view(a, "chunks", np.int32, (B,))
    out = np_view(a, "out", np.float32, (B, D))
    res = np_view(a, "result", np.int32, (B, 2))
    if fault == "writes_before_refusing":
        out[0, 0] = 0.0
    if ws_bytes < NEED:
        return -12
    start = a.views["ws"][0]
    mem = a.mem.numpy()
    counters = mem[start:start + COUNTERS].view(np.uint32)
    w = mem[start + COUNTERS:start + COUNTERS + B * 8].view(np.float32).reshape(B, 2)
    partial = mem[start + COUNTERS + B * 8:start + NEED].view(np.float32).reshape(B, 2, D)
    counters[TICKET] += 1
    for b in range(B):
        n = int(chunks[b])
        for c in range(n):
            partial[b, c] = x[b, c]
            w[b, c] = 1.0 / n
            counters[b] += 1
        if n == 0:
            out[b] = 0.0
        elif fault == "zero_weight_times_stale":
            ww = np.where(np.arange(2) < n, w[b], 0.0).astype(np.float32)       # masks the WEIGHT, multiplies the stale row
            with np.errstate(invalid="ignore"):
                out[b] = ww[0] * partial[b, 0] + ww[1] * partial[b, 1]
        else:
            out[b] = sum(w[b, c] * partial[b, c] for c in range(n))
        if fault == "reads_unwritten_byte" and n == 1:
            out[b, 0] += np.float32(mem[start + COUNTERS + B * 8 + ((b * 2 + 1) * D) * 4])   # a byte of the stale row
        counters[b] = 1 if fault == "counter_left" and b == 2 else 0
        res[b, 1] = b
    counters[TICKET] = 3 if fault == "ticket_left" else 0
    if fault == "one_past":
        mem[start + NEED] ^= 0xFF
    if fault == "one_before":
        mem[start - 1] ^= 0xFF
    if fault == "constant_guard":
        g = a.views["result"][0] - 64                          # the neighbour's guard, "restored" to a constant
        mem[g:g + 32] = mem[g]
    if fault == "copied_guard":
        g = a.views["result"][0] - 1024                        # ... or from a copy taken 256 bytes further on
        mem[g:g + 32] = mem[g + 256:g + 288]
    if fault == "wrong_column":
        res[1, 0] = 1
    return 0


def protocol(a, fault=None):
    images = sf.save(a, ["out", "result"])
    first, high = sf.run_under_fills(a, "ws", lambda: kernel(a, NEED, fault), images, ["out", "result"],
                                     other=lambda: kernel(a, NEED), what=str(fault))
    a.assert_column_is("result", torch.int32, B, 2, 0, -7, what=str(fault))
    assert np.isfinite(first["out"].view(np.float32)).all()
    return first, high


def test_a_correct_stand_in_passes():
    a, x, chunks = make()
    first, high = protocol(a)
    out = first["out"].view(np.float32).reshape(B, D)
    # the stand-in's own fp32 operations, in its order: the comparison is exact
    want = np.stack([sum(np.float32(1.0 / n) * x[b, c] for c in range(n)) if n else np.zeros(D, np.float32)
                     for b, n in enumerate(chunks)]).astype(np.float32)
    sf.assert_same_bits(first["out"], sf.bits(torch.from_numpy(want)), "the correct stand-in")
    assert (out != SENTINEL).all()
    # the last row has one chunk: its second partial row, the end of the body, stays poisoned
    assert high == NEED - D * 4
    seen = sf.run_ladder(a, "ws", [0, COUNTERS, NEED - 256, NEED], lambda n: kernel(a, n), sf.save(a, ["out", "result"]),
                         ["out", "result"], first, what="ladder")
    assert seen == [(0, -12), (COUNTERS, -12), (NEED - 256, -12), (NEED, 0)]


@pytest.mark.parametrize("fault, says", [
    ("one_past", r"1 guard byte\(s\) changed, the first 0 byte\(s\) past the end of view 'ws'"),
    ("one_before", r"1 guard byte\(s\) changed, the first 1 byte\(s\) before view 'ws'"),
    ("constant_guard", r"guard byte\(s\) changed, the first 6[0-4] byte\(s\) before view 'result'"),
    ("copied_guard", r"guard byte\(s\) changed, the first 102[0-4] byte\(s\) before view 'result'"),
    ("reads_unwritten_byte", r"output 'out' with the scratch body ff against zero"),
    ("zero_weight_times_stale", r"output 'out' with the scratch body ff against zero"),
    ("counter_left", r"view 'ws' is not zero in \[0, 65536\).*32-bit word 2\)"),
    ("ticket_left", r"view 'ws' is not zero in \[0, 65536\).*32-bit word 16383\)"),
    ("wrong_column", r"column 0 of 'result' was written"),
])
def test_a_wrong_stand_in_is_rejected(fault, says):
    a, _, _ = make()
    with pytest.raises(AssertionError, match=says):
        protocol(a, fault)


def test_nan_survives_a_zero_weight():
    """What the 0xFF fill is for: the stale row times a zero weight is NaN, and only under that fill."""
    a, _, _ = make()
    a.fill("ws", "ff", lo=COUNTERS)
    assert kernel(a, NEED, "zero_weight_times_stale") == 0
    out = a.view("out", torch.float32).view(B, D).numpy()
    assert np.isnan(out[1]).all() and np.isnan(out[4]).all() and np.isfinite(out[[0, 2, 3]]).all()
    a.fill("ws", "zero")
    assert kernel(a, NEED, "zero_weight_times_stale") == 0
    assert np.isfinite(a.view("out", torch.float32).numpy()).all()


def test_a_refusal_that_wrote_is_rejected():
    a, _, _ = make()
    first, _ = protocol(a)
    with pytest.raises(AssertionError, match=r"refused 0 bytes with status -12: \d+ byte\(s\) of the arena changed, the first "
                                             r"inside view 'out' at byte"):
        sf.run_ladder(a, "ws", [0, NEED], lambda n: kernel(a, n, "writes_before_refusing"), sf.save(a, ["out", "result"]),
                      ["out", "result"], first, what="ladder")


def test_the_fence_stands_behind_the_bytes_given():
    """A view told to be smaller than its extent: the first byte behind it is guard, and the arena owns the extent."""
    a, _, _ = make()
    a.resize("ws", NEED - 256)
    a.assert_guards_intact()
    start = a.views["ws"][0]
    assert start + NEED + sf.GUARD <= a.capacity
    a.mem[start + NEED - 256] ^= 0xFF
    with pytest.raises(AssertionError, match=r"the first 0 byte\(s\) past the end of view 'ws'"):
        a.assert_guards_intact()


def test_layout():
    a, _, _ = make()
    starts = sorted((s, n, e) for s, n, e in a.views.values())
    assert all(s % sf.ALIGN == 0 and a.address(name) % sf.ALIGN == 0 for name, (s, _, _) in a.views.items())
    assert starts[0][0] >= sf.GUARD
    for (s0, n0, e0), (s1, _, _) in zip(starts, starts[1:]):
        assert s1 - (s0 + max(n0, e0)) >= sf.GUARD
    assert a.capacity - (starts[-1][0] + starts[-1][2]) >= sf.GUARD
    # inputs are followed by 0xFF, everything else by the positional pattern, which is never 0x00 or 0xFF
    s, n, _ = a.views["x"]
    assert (a.mem[s + n:s + n + sf.GUARD] == 0xFF).all()
    p = sf.pattern(0, 1 << 16, "cpu")
    assert p.min() > 0 and p.max() < 0xFF and not (p[:-256] == p[256:]).all() and len(torch.unique(p[:4096])) > 200
    assert int(a.ptr("ws").value) == a.address("ws")
    a.resize("ws", 0)
    assert int(a.ptr("ws").value) == a.address("ws") and a.view("ws").numel() == 0
