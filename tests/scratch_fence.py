"""An arena with fences for the scratch contract of include/mli_kernels.h.

One torch.uint8 allocation per case.  The whole arena starts as a position-dependent byte pattern; carve() punches
256-byte-aligned views out of it, at least GUARD bytes apart, so every byte that is not inside a view is a guard and
assert_guards_intact() checks all of them in one comparison.  A view may be shorter than the extent reserved for it
(a scratch buffer the call is told is smaller than it needs): the guard then begins directly behind the bytes given and
the arena still owns the full extent plus a guard, so an overrun lands in memory the test owns and shows.

Fills: "zero" (all zero bytes), "ff" (0xFF: NaN as fp32 and as bf16, -1 as a counter), "keep" (what the previous call
left).  A view carved with tail="ff" (inputs) is followed by a guard of 0xFF instead of the pattern, so a read past the
input's end that reaches a result shows as NaN; that guard is checked like every other.

Works on CPU tensors too (tests/test_scratch_fence_cpu.py proves there that every check bites).
TEST INFRASTRUCTURE: never used by the product."""
import ctypes

import numpy as np
import torch

GUARD = 4096     # bytes between two views, and behind the last one
ALIGN = 256      # alignment of every view
POISON = 0xFF
FILLS = ("zero", "ff", "keep")


def pattern(lo, hi, device):
    """Guard byte of arena offsets lo .. hi - 1: a function of the offset whose period is not a power of two, so a block
    copied from another place, or a constant, differs."""
    i = torch.arange(lo, hi, dtype=torch.int64, device=device)
    return ((i * 167 + (i >> 8) * 13 + 0x5A) % 251 + 2).to(torch.uint8)


def _round_up(n, a):
    return (n + a - 1) // a * a


class Arena:
    def __init__(self, capacity, device):
        self.device = torch.device(device)
        self.capacity = _round_up(int(capacity), ALIGN) + GUARD
        self.buf = torch.empty(self.capacity + ALIGN, dtype=torch.uint8, device=self.device)
        self._skew = (-self.buf.data_ptr()) % ALIGN          # offset 0 of the arena is 256-byte aligned in memory
        self.mem = self.buf[self._skew:self._skew + self.capacity]
        self.mem.copy_(pattern(0, self.capacity, self.device))
        self._is_guard = torch.ones(self.capacity, dtype=torch.bool, device=self.device)
        self._is_ff = torch.zeros(self.capacity, dtype=torch.bool, device=self.device)
        self.views = {}      # name -> [start, nbytes, extent]
        self._cursor = GUARD

    # ---- layout ---------------------------------------------------------------------------------------------------
    @staticmethod
    def room(*sizes):
        """Capacity for views of these sizes (extents)."""
        return GUARD + sum(_round_up(int(n), ALIGN) + GUARD + ALIGN for n in sizes)

    def carve(self, name, nbytes, fill="zero", extent=None, tail="pattern"):
        """A view of nbytes bytes; the arena owns max(nbytes, extent) + GUARD bytes from its start."""
        assert name not in self.views and fill in FILLS[:2] and tail in ("pattern", "ff"), (name, fill, tail)
        nbytes = int(nbytes)
        extent = max(nbytes, int(extent or 0))
        start = self._cursor
        end = start + extent + GUARD
        assert end <= self.capacity, f"arena too small for {name}: {end} > {self.capacity}"
        self.views[name] = [start, nbytes, extent]
        self._cursor = _round_up(end, ALIGN)
        self._is_guard[start:start + nbytes] = False
        if tail == "ff":
            self._is_ff[start + nbytes:start + nbytes + GUARD] = True
            self.mem[start + nbytes:start + nbytes + GUARD] = POISON
        self.fill(name, fill)
        return self.view(name)

    def resize(self, name, nbytes):
        """Move the fence of a view: it now has nbytes bytes (<= its extent); what lies behind them is guard again."""
        start, old, extent = self.views[name]
        nbytes = int(nbytes)
        assert 0 <= nbytes <= extent, (name, nbytes, extent)
        self.views[name][1] = nbytes
        self._is_guard[start:start + extent] = True
        self._is_guard[start:start + nbytes] = False
        self.mem[start + nbytes:start + extent] = pattern(start + nbytes, start + extent, self.device)
        return self.view(name)

    def view(self, name, dtype=torch.uint8, shape=None):
        start, nbytes, _ = self.views[name]
        v = self.mem[start:start + nbytes].view(dtype)
        return v if shape is None else v.view(shape)

    def ptr(self, name, offset=0):
        """What crosses the C ABI: the address of the view (valid for a view of 0 bytes too)."""
        return ctypes.c_void_p(self.mem.data_ptr() + self.views[name][0] + offset)

    def address(self, name):
        return self.mem.data_ptr() + self.views[name][0]

    def put(self, name, array):
        """Copy a numpy array or a tensor into a view of exactly its size."""
        t = torch.from_numpy(np.ascontiguousarray(array)) if isinstance(array, np.ndarray) else array.contiguous()
        raw = t.reshape(-1).view(torch.uint8)
        v = self.view(name)
        assert raw.numel() == v.numel(), (name, raw.numel(), v.numel())
        v.copy_(raw)

    def carve_from(self, name, array, tail="ff"):
        """An input: a view holding `array`, followed by a 0xFF guard."""
        n = array.nbytes if isinstance(array, np.ndarray) else array.numel() * array.element_size()
        self.carve(name, n, "zero", tail=tail)
        self.put(name, array)
        return self.view(name)

    def fill(self, name, fill, lo=0, hi=None):
        assert fill in FILLS, fill
        if fill == "keep":
            return
        start, nbytes, _ = self.views[name]
        hi = nbytes if hi is None else min(int(hi), nbytes)
        if lo < hi:
            self.mem[start + lo:start + hi] = 0 if fill == "zero" else POISON

    # ---- checks ---------------------------------------------------------------------------------------------------
    def _where(self, offset):
        """Names the view an arena offset lies in, or the nearer of the view that ends before it and the one that starts
        behind it."""
        past = before = None
        for name, (start, nbytes, _) in self.views.items():
            if start <= offset < start + nbytes:
                return f"inside view {name!r} at byte {offset - start}"
            if offset >= start + nbytes and (past is None or offset - start - nbytes < past[0]):
                past = (offset - start - nbytes, f"{offset - start - nbytes} byte(s) past the end of view {name!r} "
                                                 f"(its byte {offset - start})")
            if offset < start and (before is None or start - offset < before[0]):
                before = (start - offset, f"{start - offset} byte(s) before view {name!r}")
        return min([c for c in (past, before) if c is not None] or [(0, f"at arena offset {offset}")])[1]

    def _expected_guard(self):
        want = pattern(0, self.capacity, self.device)
        want[self._is_ff] = POISON
        return want

    def assert_guards_intact(self, what=""):
        """One device-side comparison and one sync; names the view and the offset of the first changed byte."""
        bad = (self.mem != self._expected_guard()) & self._is_guard
        n = int(bad.sum())                                   # the one sync
        if n:
            first = int(torch.nonzero(bad)[0])
            raise AssertionError(f"{what}: {n} guard byte(s) changed, the first {self._where(first)}: "
                                 f"holds {int(self.mem[first]):#04x}")

    def snapshot(self):
        return self.mem.clone()

    def assert_unchanged(self, snap, what=""):
        """Not one byte of the arena differs from the snapshot."""
        bad = self.mem != snap
        n = int(bad.sum())
        if n:
            first = int(torch.nonzero(bad)[0])
            raise AssertionError(f"{what}: {n} byte(s) of the arena changed, the first {self._where(first)}")

    def high_water(self, name, fill, lo=0):
        """Bytes from the start of the view up to and including the last byte (at or after lo) that no longer holds the
        poison of `fill`; lo if every byte from lo on still does."""
        assert fill in ("zero", "ff")
        v = self.view(name)[lo:]
        touched = torch.nonzero(v != (0 if fill == "zero" else POISON))
        return lo + (int(touched[-1]) + 1 if touched.numel() else 0)

    def assert_zero(self, name, lo=0, hi=None, what=""):
        v = self.view(name)
        hi = v.numel() if hi is None else hi
        assert hi <= v.numel(), (name, hi, v.numel())
        nz = torch.nonzero(v[lo:hi])
        if nz.numel():
            first = lo + int(nz[0])
            raise AssertionError(f"{what}: view {name!r} is not zero in [{lo}, {hi}): {nz.numel()} byte(s), the first at "
                                 f"byte {first} (32-bit word {first // 4}) holds {int(v[first]):#04x}")

    def assert_column_is(self, name, dtype, rows, n_cols, col, sentinel, what=""):
        """Column `col` of the view read as [rows, n_cols, width] of `dtype` holds `sentinel` bit for bit (a column the
        call was not asked to write)."""
        t = self.view(name, dtype).view(rows, n_cols, -1)[:, col].contiguous()
        want = torch.full_like(t, sentinel)
        bad = torch.nonzero((t.view(torch.uint8) != want.view(torch.uint8)).reshape(-1))
        if bad.numel():
            raise AssertionError(f"{what}: column {col} of {name!r} was written: {bad.numel()} byte(s) differ from the "
                                 f"sentinel, the first at byte {int(bad[0])} of the column")


def bits(t):
    """The raw bytes of a tensor, as a host numpy array: what 'bit-identical' compares."""
    return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().copy()


def assert_same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero(got != want)[0]
    assert not len(bad), f"{what}: {len(bad)} byte(s) differ, the first at byte {int(bad[0])}"


# ---- the protocol of a scratch case ---------------------------------------------------------------------------------------
COUNTER_BYTES = 65536    # the arrival counters in front of an attention workspace (include/mli_kernels.h)


def save(arena, names):
    """Images of views a call changes (outputs at their sentinel, pages, lengths), to put back before every call."""
    return {n: arena.view(n).clone() for n in names}


def restore(arena, images):
    for n, img in images.items():
        arena.view(n).copy_(img)


def output_bits(arena, outputs):
    return {n: bits(arena.view(n)) for n in outputs}


def run_under_fills(arena, scratch, call, images, outputs, other=None, counters=COUNTER_BYTES, what=""):
    """The call under the three fills of the scratch body: "zero", "ff", and "keep" after `other` (a different call) used
    the same scratch.  call() and other() return the entry point's status.  The counter region is zeroed here, once, and
    never again.  After every call: status 0, every guard intact, the counter region zero; the outputs of the three
    runs are bit-identical.  Returns (bits of the outputs, high-water mark of the 0xFF run in bytes)."""
    arena.fill(scratch, "zero")
    first, high = None, None
    for fill in FILLS:
        if fill == "keep":
            if other is None:
                continue
            rc = other()
            assert rc == 0, f"{what}: the other call returned {rc}"
            arena.assert_guards_intact(f"{what}, the other call")
            if counters:
                arena.assert_zero(scratch, 0, counters, f"{what}, counters after the other call")
        else:
            arena.fill(scratch, fill, lo=counters)
        restore(arena, images)
        rc = call()
        assert rc == 0, f"{what}, body {fill}: status {rc} with exactly the bytes the size function asks for"
        arena.assert_guards_intact(f"{what}, body {fill}")
        if counters:
            arena.assert_zero(scratch, 0, counters, f"{what}, body {fill}: counters after the call")
        got = output_bits(arena, outputs)
        if fill == "ff":
            high = arena.high_water(scratch, "ff", lo=counters)
        if first is None:
            first = got
        else:
            for n in outputs:
                assert_same_bits(got[n], first[n], f"{what}: output {n!r} with the scratch body {fill} against zero")
    return first, high


def run_ladder(arena, scratch, sizes, call, images, outputs, want, counters=COUNTER_BYTES, what=""):
    """The call with a valid pointer and each of `sizes` bytes in rising order, the fence directly behind them and the body
    0xFF.  The counter region is zeroed once, at the first rung that holds all of it (the smaller rungs leave guard bytes
    where it will be), and never again: a refusal changes nothing and a success leaves it zero.  A negative status: not one
    byte of the arena changed.  Status 0: guards intact, counters zero, the bits of the full-size run (`want`).  Anything
    else fails.  Returns [(bytes, status)]."""
    seen = []
    arena.resize(scratch, 0)
    zeroed = False
    for n in sorted({max(int(s), 0) for s in sizes}):
        arena.resize(scratch, n)
        if counters and n >= counters and not zeroed:
            arena.fill(scratch, "zero", 0, counters)
            zeroed = True
        arena.fill(scratch, "ff", lo=counters)
        restore(arena, images)
        before = arena.snapshot()
        rc = call(n)
        seen.append((n, rc))
        if rc < 0:
            arena.assert_unchanged(before, f"{what}: refused {n} bytes with status {rc}")
            continue
        assert rc == 0, f"{what}: status {rc} with {n} bytes"
        arena.assert_guards_intact(f"{what}, {n} bytes")
        if counters and n >= counters:
            arena.assert_zero(scratch, 0, counters, f"{what}, {n} bytes: counters")
        got = output_bits(arena, outputs)
        for name in outputs:
            assert_same_bits(got[name], want[name], f"{what}: output {name!r} with {n} bytes against the full-size run")
    return seen
