"""mli_paged_prefill_window (ops.paged_prefill(window=, sinks=)): the prefill of the live tokens of rows that decode under a
sliding window with attention sinks (csrc/page_live.hpp).

For every page element type, both prefill forms and both fill grids: the live pages of the new rows receive the bits
mli_paged_prefill writes to them on a full table; the table entry of a dead page is never followed (it names a canary page,
or is null) and no other byte of the pool -- dead pages, canaries, guard bytes, rows that are not new -- changes.  Windows
that leave no row a dead page are mli_paged_prefill."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAGE = 16
F32, BF16, FP8 = 0, 1, 2
ESIZE = {F32: 4, BF16: 2, FP8: 1}
N_CANARY = 3


def _dead(page, n, W, K):
    """The rule, restated: page i of a row of n tokens is dead iff ceil(K / 16) <= i < max(0, n - W) // 16."""
    return -(-K // PAGE) <= page < max(0, n - W) // PAGE


def _lengths(S, W, K):
    """0, 1, W, W + 1, a length whose window starts on a page edge, one with p0 == ps (no gap), one with a gap of exactly
    one page, and S."""
    ps = -(-K // PAGE)
    return [0, 1, W, W + 1, W + 5 * PAGE, W + PAGE * ps + 7, W + PAGE * (ps + 1) + 3, S]


class _Case:
    """A pool of B * S / 16 pages between two guard pages and N_CANARY canary pages behind, as bytes; the full table; and the
    inputs of one prefill call."""

    def __init__(self, dev, seed, B, S, D, elem, lengths, new_idx, V=300):
        rng = np.random.default_rng(seed)
        self.dev, self.B, self.S, self.D, self.elem = dev, B, S, D, elem
        self.npages = S // PAGE
        self.page_bytes = PAGE * 3 * D * ESIZE[elem]
        n = B * self.npages
        # random bytes everywhere (fp32 / bf16 NaN patterns included: nothing may depend on what a page held)
        self.initial = rng.integers(0, 256, size=(1 + n + N_CANARY + 1) * self.page_bytes, dtype=np.uint8)
        self.full = (1 + np.arange(n, dtype=np.int64).reshape(B, self.npages)) * self.page_bytes   # byte offsets
        self.canary = (1 + n + np.arange(N_CANARY, dtype=np.int64)) * self.page_bytes
        self.lengths = np.asarray(lengths, np.int32)
        self.new_idx = np.asarray(new_idx, np.int32)
        emb = (rng.random((V, D), dtype=np.float32) * 2 - 1).astype(np.float32)
        wpe = (rng.random((S, D), dtype=np.float32) * 2 - 1).astype(np.float32)
        inp = rng.integers(0, V, size=(B, S)).astype(np.int32)
        w = [((rng.random((D, D), dtype=np.float32) * 2 - 1) / np.sqrt(D)).astype(np.float32) for _ in range(2)]
        t = lambda a: torch.from_numpy(a).to(dev)
        self.args = (t(emb), t(wpe), t(inp))
        self.w = [t(x) if elem == F32 else t(x).to(torch.bfloat16) for x in w]
        self.d_len, self.d_idx = t(self.lengths), t(self.new_idx)

    def run(self, table, **kw):
        """One prefill over a fresh copy of the pool with `table` (byte offsets; < 0 = null); returns the pool's bytes."""
        from min_llm_inference_amd import ops
        pool = torch.from_numpy(self.initial.copy()).to(self.dev)
        ptrs = torch.from_numpy(np.where(table >= 0, pool.data_ptr() + table, 0).astype(np.int64)).to(self.dev)
        ops.paged_prefill(*self.args, ptrs, self.d_len, self.d_idx, self.w[0], self.w[1], len(self.new_idx), elem=self.elem, **kw)
        torch.cuda.synchronize()
        return pool.cpu().numpy()

    def dead_entries(self, W, K):
        return np.array([[_dead(i, min(int(self.lengths[b]), self.S), W, K) for i in range(self.npages)] for b in range(self.B)])

    def expected(self, reference, W, K):
        """The initial bytes, with the live pages of the new rows taken from the un-windowed prefill's pool."""
        want = self.initial.copy()
        dead = self.dead_entries(W, K)
        for b in self.new_idx:
            for i in range(self.npages):
                if not dead[b, i]:
                    o = self.full[b, i]
                    want[o:o + self.page_bytes] = reference[o:o + self.page_bytes]
        return want


def _check_window(c, W, K):
    reference = c.run(c.full)
    assert (reference != c.initial).any()
    dead = c.dead_entries(W, K)
    want = c.expected(reference, W, K)
    assert dead[c.new_idx].any(), "the case has no dead page"
    # dead entries name canary pages (other rows' pages, for all the kernel can tell)
    canaries = c.canary[np.arange(dead.size).reshape(dead.shape) % N_CANARY]
    got = c.run(np.where(dead, canaries, c.full), window=W, sinks=K)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at page {bad[0] // c.page_bytes - 1} (+{bad[0] % c.page_bytes})"
    # ... or are null
    got = c.run(np.where(dead, -1, c.full), window=W, sinks=K)
    assert np.array_equal(got, want), "dead entries null"


CONFIGS = [  # elem, D, B
    pytest.param(F32, 64, 6, id="f32-64"), pytest.param(F32, 128, 6, id="f32-128"),
    pytest.param(BF16, 128, 6, id="bf16-128"), pytest.param(BF16, 512, 6, id="bf16-512"),
    pytest.param(FP8, 128, 6, id="fp8-128"),
    pytest.param(F32, 2048, 4, id="f32-2048-two-launches"),
]
WINDOWS = [(12, 0), (40, 4), (17, 16), (16, 32)]


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("W,K", WINDOWS)
@pytest.mark.parametrize("elem,D,B", CONFIGS)
def test_live_pages_match_and_nothing_else_changes(mli, dev, elem, D, B, W, K, half):
    S = 256
    four = _lengths(S, W, K)[half::2]            # half 0: 0, W, page edge, one-page gap; half 1: 1, W + 1, no gap, S
    rng = np.random.default_rng(1000 + W + K + half)
    new_idx = rng.permutation(B)[:4]
    lengths = np.full((B,), S - 9, np.int32)      # rows that are not new: long, and left alone
    lengths[new_idx] = four
    _check_window(_Case(dev, 7 * D + W + half, B, S, D, elem, lengths, new_idx), W, K)


@pytest.mark.parametrize("fused", [2, 0])
@pytest.mark.parametrize("elem,D", [(F32, 64), (BF16, 128), (FP8, 128)])
def test_per_row_grid_and_both_forms(mli, dev, elem, D, fused):
    """mli_tune "fill_compact" = 0: one tile grid per new row, where a tile wholly in dead pages leaves and a dead token of a
    mixed tile is dropped; "prefill_fused" = 2 / 0: the prologue form / encoder + fill at a width that takes the other by
    default (bf16 with the fp32-widened fill as well)."""
    S, B, W, K = 256, 6, 40, 4
    lengths = np.array([S, 1, W + PAGE * 2 + 3, 0, 200, 131], np.int32)
    new_idx = np.array([4, 0, 2, 5], np.int32)
    c = _Case(dev, 99 + D, B, S, D, elem, lengths, new_idx)
    assert mli.mli_tune(b"fill_compact", 0) == 0 and mli.mli_tune(b"prefill_fused", fused) == 0
    try:
        _check_window(c, W, K)
        if elem == BF16:
            assert mli.mli_tune(b"bf16_native_mfma", 0) == 0
            _check_window(c, W, K)
            mli.mli_tune(b"fill_compact", 1)
            _check_window(c, W, K)
    finally:
        mli.mli_tune(b"fill_compact", 1)
        mli.mli_tune(b"prefill_fused", 1)
        mli.mli_tune(b"bf16_native_mfma", 1)


@pytest.mark.parametrize("elem,D", [(F32, 64), (BF16, 128), (FP8, 128)])
@pytest.mark.parametrize("W,K", [(256, 0), (300, 4), (200, 56), (16, 240), (0, 5)])
def test_windows_without_a_dead_page_are_the_plain_prefill(mli, dev, elem, D, W, K):
    """W >= S, K + W >= S (and no window at all): mli_paged_prefill's bits on every page."""
    S, B = 256, 6
    lengths = np.array([S, 1, 100, 0, 255, 17], np.int32)
    c = _Case(dev, 5 + D, B, S, D, elem, lengths, np.array([5, 0, 2, 4], np.int32))
    assert np.array_equal(c.run(c.full, window=W, sinks=K), c.run(c.full))


def test_more_new_rows_than_the_flat_list_holds(mli, dev):
    """n_new = 2049 > kMaxCompactRows: the per-row grid without a tuning switch."""
    S, D, W, B = 64, 64, 12, 2049
    rng = np.random.default_rng(77)
    lengths = rng.integers(0, S + 1, size=B).astype(np.int32)
    lengths[:4] = [S, 0, W + PAGE, W + 2 * PAGE + 1]
    _check_window(_Case(dev, 78, B, S, D, F32, lengths, rng.permutation(B)), W, 0)
