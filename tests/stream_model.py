"""The equal-page-shares scan's PARTITION (csrc/attention_stream.hip), restated in plain Python from the kernel's header
comment and launch_stream_decode, the length vectors that place row boundaries against share boundaries, and a float64
attention evaluated piece by piece the way the kernel does it.  Shared by tests/test_stream_model_cpu.py (which proves
that the vectors reach every partition event and that the comparison sees eight partition bugs) and
tests/test_stream_partition_gpu.py (which runs the vectors through the kernel).

The contract: the pages of all rows form one sequence (row 0's pages, row 1's, ...; a row of L tokens has
ceil(min(L, S) / 16) pages), P pages in all.  G = min(G_launch, max(1, P // 16)) workgroups share it.  With a dynamic part
of dyn_pct per cent in granules of `gran` pages -- on only when P * dyn_pct // 100 >= gran -- the first
Ps = P - P * dyn_pct // 100 pages are cut into G static shares [w Ps // G, (w + 1) Ps // G) and the rest into granules
[Ps + k gran, min(Ps + (k + 1) gran, P)).  Every piece yields one (m, l, partial) triple per row it meets; a row's
triples are merged in page order -- static shares first, then granules -- once all of them have arrived; a row that
meets one piece is written directly; a row without pages is zero.

Nothing here is derived from the kernel's row_triples(): how many pieces meet a row is counted by intersecting."""
import math
from types import SimpleNamespace

import numpy as np

from helpers import PAGE

MIN_PAGES = 16            # a share is never shorter than this many pages: fewer workgroups share then
MAX_ROWS = 2048           # rows whose page counts fit the kernel's prefix array
SENTINEL = 12345.0        # what a row keeps whose triples never all arrive
# (dyn_pct, granule): production first, static shares only, the two splits of the older tests, the largest granule
SPLITS = ((4, 64), (0, 64), (12, 16), (60, 16), (4, 256))

# by name, so that the GPU test can be laid out without a device (tests/test_stream_model_cpu.py holds them to the vectors):
PEAK_VECTORS = ("one_row_per_share", "shifted_by_one_page", "full_rows", "full_rows_to_S", "sparse", "tiny")   # rows in >= 2 pieces
OFFSET_VECTORS = ("full_rows", "sparse")
SMALL_VECTORS = ("full_rows", "full_rows_to_S", "one_page_rows", "sparse", "tiny")     # P <= 2048 pages: also at wide rows
N_ARRAYS = {"one_row_per_share": 1, "shifted_by_one_page": 1, "full_rows": 1, "full_rows_to_S": 1, "one_page_rows": 1,
            "sparse": 2, "tiny": 6}

EVENTS = (
    "no_pages",                    # P == 0
    "one_workgroup",               # G == 1
    "fewer_workgroups",            # G < G_launch
    "dynamic_on",
    "dynamic_too_small",           # dyn_pct > 0 but P * dyn_pct // 100 < gran: static shares only
    "static_cut_on_row_start",     # a boundary between two static shares is the first page of a row
    "granule_cut_on_row_start",    # a granule's first page is the first page of a row
    "row_whole",                   # a row inside one piece: written directly
    "row_in_2_pieces",
    "row_in_4_or_more_pieces",
    "row_is_whole_shares",         # a row in two or more static shares that starts and ends on their boundaries
    "row_static_and_dynamic",      # a row that ends in the static part and continues in a granule
    "granule_straddles_rows",
    "last_granule_short",
    "piece_under_4_pages",         # waves without a page
    "more_rows_than_maxseg",       # a piece whose rows need more than one group
    "empty_row_in_piece",
    "empty_run_over_maxseg",       # a run of empty rows inside a piece longer than a group
    "leading_empty_row",
    "trailing_empty_row",
    "row_of_length_S",
)


def page_counts(lengths, S):
    L = np.clip(np.asarray(lengths).astype(np.int64), 0, S)
    return (L + PAGE - 1) // PAGE


def partition(lengths, S, G_launch, dyn_pct, gran):
    """P, G, Ps, n_gran, pieces [(lo, hi, kind)] in page order (kind "static" / "granule"; empty pieces left out),
    row_pieces[b] = number of pieces that meet row b, and start[b] .. start[b + 1] = the pages of row b."""
    pages = page_counts(lengths, S)
    start = np.concatenate([[0], np.cumsum(pages)]).astype(np.int64)
    P = int(start[-1])
    if P == 0:
        return SimpleNamespace(P=0, G=0, Ps=0, n_gran=0, pieces=[], row_pieces=np.zeros(len(pages), np.int64), start=start,
                               S=S, G_launch=G_launch, dyn_pct=dyn_pct, gran=gran)
    G = min(G_launch, max(1, P // MIN_PAGES))
    dyn = P * dyn_pct // 100 if dyn_pct > 0 else 0
    Ps = P - dyn if dyn >= gran else P
    n_gran = -(-(P - Ps) // gran)
    pieces = [(w * Ps // G, (w + 1) * Ps // G, "static") for w in range(G)]
    pieces += [(Ps + k * gran, min(Ps + (k + 1) * gran, P), "granule") for k in range(n_gran)]
    pieces = [p for p in pieces if p[1] > p[0]]
    row_pieces = np.zeros(len(pages), np.int64)
    for lo, hi, _ in pieces:
        for b in rows_of_piece(start, lo, hi):
            row_pieces[b] += 1
    return SimpleNamespace(P=P, G=G, Ps=Ps, n_gran=n_gran, pieces=pieces, row_pieces=row_pieces, start=start, S=S,
                           G_launch=G_launch, dyn_pct=dyn_pct, gran=gran)


def rows_of_piece(start, lo, hi):
    """The rows with a page in [lo, hi), ascending."""
    first = int(np.searchsorted(start, lo, side="right")) - 1      # the last row that starts at or before lo ...
    out = []
    for b in range(first, len(start) - 1):
        if start[b] >= hi:
            break
        if min(start[b + 1], hi) > max(start[b], lo):              # ... rows without pages in between drop out here
            out.append(b)
    return out


def events(lengths, S, G_launch, dyn_pct, gran, maxseg=4):
    """The partition events (names of EVENTS) a length vector reaches under one split."""
    L = np.asarray(lengths).astype(np.int64)
    pt = partition(L, S, G_launch, dyn_pct, gran)
    ev = set()
    pages = np.diff(pt.start)
    live = pages > 0
    if len(L) and not live[0]:
        ev.add("leading_empty_row")
    if len(L) and not live[-1]:
        ev.add("trailing_empty_row")
    if (L == S).any():
        ev.add("row_of_length_S")
    if pt.P == 0:
        ev.add("no_pages")
        return ev
    if pt.G == 1:
        ev.add("one_workgroup")
    if pt.G < G_launch:
        ev.add("fewer_workgroups")
    if pt.n_gran:
        ev.add("dynamic_on")
    elif dyn_pct > 0:
        ev.add("dynamic_too_small")
    row_starts = {int(s) for s in pt.start[:-1][live]}
    kinds = {b: set() for b in np.nonzero(live)[0]}
    for i, (lo, hi, kind) in enumerate(pt.pieces):
        if lo in row_starts and lo > 0:
            if kind == "granule":
                ev.add("granule_cut_on_row_start")
            elif pt.pieces[i - 1][2] == "static":
                ev.add("static_cut_on_row_start")
        rows = rows_of_piece(pt.start, lo, hi)
        for b in rows:
            kinds[b].add(kind)
        if kind == "granule":
            if len(rows) > 1:
                ev.add("granule_straddles_rows")
            if hi - lo < gran:
                ev.add("last_granule_short")
        if hi - lo < 4:
            ev.add("piece_under_4_pages")
        if rows[-1] - rows[0] + 1 > maxseg:                        # the kernel groups by row index, empty rows included
            ev.add("more_rows_than_maxseg")
        gaps = np.diff(rows) - 1
        if (gaps > 0).any():
            ev.add("empty_row_in_piece")
        if (gaps > maxseg).any():
            ev.add("empty_run_over_maxseg")
    cuts = {lo for lo, hi, kind in pt.pieces if kind == "static"} | {hi for lo, hi, kind in pt.pieces if kind == "static"}
    for b in np.nonzero(live)[0]:
        if pt.row_pieces[b] >= 2 and kinds[b] == {"static"} and int(pt.start[b]) in cuts and int(pt.start[b + 1]) in cuts:
            ev.add("row_is_whole_shares")
    n = pt.row_pieces[live]
    if (n == 1).any():
        ev.add("row_whole")
    if (n == 2).any():
        ev.add("row_in_2_pieces")
    if (n >= 4).any():
        ev.add("row_in_4_or_more_pieces")
    if any(len(k) == 2 for k in kinds.values()):
        ev.add("row_static_and_dynamic")
    return ev


def stream_vectors(G_launch, S):
    """{name: [length vectors]}: the named vectors, parametric in G_launch (2 x CUs on the chip that runs them) so that the
    alignments hold there.  Ordered: tests/test_stream_model_cpu.py asserts what each name adds to the ones before it."""
    assert S % PAGE == 0 and S >= 1024 and 16 <= G_launch <= MAX_ROWS
    i32 = lambda a: np.asarray(a, np.int32)   # noqa: E731
    v = {}
    # G_launch rows of 16 pages (241 .. 256 tokens): with static shares only, every share is one row
    rows16 = 15 * PAGE + 1 + np.arange(G_launch) % PAGE
    v["one_row_per_share"] = [i32(rows16)]
    shifted = rows16.copy()
    shifted[0] -= PAGE                        # ... and every row boundary one page before a share boundary
    v["shifted_by_one_page"] = [i32(shifted)]
    # 32 x W = 2048 pages at S = 1024: 128 shares of 16 pages, every row exactly 4 of them
    v["full_rows"] = [i32([S - 1] * 32)]
    to_S = np.full(32, S - 1)
    to_S[[0, 5, 6, 31]] = S
    v["full_rows_to_S"] = [i32(to_S)]
    v["one_page_rows"] = [i32(1 + (7 * np.arange(2048)) % PAGE)]
    # every seventh row live (runs of six empty rows); the second with row 0 and the last row empty
    rng = np.random.default_rng(7103)
    sp = np.zeros(700, np.int64)
    sp[::7] = rng.integers(1, 6 * PAGE + 1, size=100)
    sp2 = np.zeros(700, np.int64)
    sp2[3::7] = rng.integers(1, 6 * PAGE + 1, size=100)
    sp2[696] = 0
    v["sparse"] = [i32(sp), i32(sp2)]
    # P = 0, 3, 15, 16, 31, 32
    v["tiny"] = [i32([0, 0, 0]), i32([5, 0, 17]), i32([7 * PAGE, 0, 8 * PAGE]), i32([16 * PAGE]),
                 i32([15 * PAGE, 1, 15 * PAGE - 1]), i32([16 * PAGE, 16 * PAGE - 1])]
    for name, group in v.items():
        for L in group:
            assert len(L) <= MAX_ROWS and L.min() >= 0 and L.max() <= S, name
    return v


def piece_maxima(x, lengths, pt):
    """{row: [max score of the row's tokens in each piece that meets it, in page order]} for the rows in two or more pieces,
    from scores x [B, >= longest row] (f64_model.Model.x): the `m` of the triples the kernel leaves in its workspace."""
    L = np.clip(np.asarray(lengths).astype(np.int64), 0, pt.S)
    out = {}
    for lo, hi, _ in pt.pieces:
        for b in rows_of_piece(pt.start, lo, hi):
            if pt.row_pieces[b] >= 2:
                t0 = (max(int(pt.start[b]), lo) - int(pt.start[b])) * PAGE
                t1 = min((min(int(pt.start[b + 1]), hi) - int(pt.start[b])) * PAGE, int(L[b]))
                out.setdefault(b, []).append(float(x[b, t0:t1].max()))
    return out


# ---- float64 attention, piece by piece ---------------------------------------------------------------------------------
MUTANTS = (
    "share_drops_last_page",        # a static share stops one page early
    "cut_page_to_previous_row",     # a page at a share boundary that is also a row start goes to the row before
    "arrivals_one_too_many",        # a row that ends on a share boundary waits for a triple that never comes
    "granule_slot_on_last_static",  # the first granule's slot is n_static - 1: it overwrites the last static triple
    "last_granule_skipped",         # the last, partial granule is never processed
    "first_maxseg_rows_only",       # only the first group of a piece's rows is processed
    "empty_rows_shift_q",           # empty rows inside a piece shift the q row of the rows behind them
    "merge_without_rescale",        # triples merged without exp(m_i - m)
    "length_S_as_S_minus_1",        # a row of S tokens loses its last one
)


def piecewise_attention(q, kt, v, lengths, pt, mutant=None, maxseg=4, cache=None):
    """[B, D] float64 attention evaluated the way the kernel does it under partition `pt`: every piece produces one
    (m, l, partial) triple per row it meets, stored in the row's slot for that piece -- static shares in order, then
    granules -- and the row is merged when as many triples have arrived as pieces meet it; rows with one piece are
    written directly; rows whose expected count is never reached keep SENTINEL.  `mutant` (one of MUTANTS) puts one
    partition bug in.  `cache` (a dict) shares the triples of identical token ranges between calls on the same inputs."""
    assert mutant is None or mutant in MUTANTS, mutant
    B, D = np.shape(q)
    S = pt.S
    L = np.clip(np.asarray(lengths).astype(np.int64), 0, S)
    if mutant == "length_S_as_S_minus_1":
        L = np.where(L == S, S - 1, L)
    start = pt.start
    live = np.diff(start) > 0
    out = np.full((B, D), SENTINEL, np.float64)
    out[~live] = 0.0
    cache = {} if cache is None else cache
    scale = 1.0 / math.sqrt(D)

    def triple(q_row, kv_row, t0, t1):
        key = (q_row, kv_row, t0, t1)
        if key not in cache:
            x = (np.asarray(q[q_row]).astype(np.float64) @ np.asarray(kt[kv_row, :, t0:t1]).astype(np.float64)) * scale
            m = x.max()
            e = np.exp(x - m)
            cache[key] = (m, e.sum(), e @ np.asarray(v[kv_row, t0:t1]).astype(np.float64))
        return cache[key]

    def merged(triples, rescale=True):
        m = max(t[0] for t in triples)
        wgt = [math.exp(t[0] - m) if rescale else 1.0 for t in triples]
        l = sum(t[1] * w for t, w in zip(triples, wgt))
        return sum(t[2] * w for t, w in zip(triples, wgt)) / l

    # the work of every piece: (row the triple goes to, q row, K / V row, first page, last page + 1)
    work = []
    for i, (lo, hi, kind) in enumerate(pt.pieces):
        if mutant == "share_drops_last_page" and kind == "static":
            hi -= 1
        if mutant == "last_granule_skipped" and kind == "granule" and i == len(pt.pieces) - 1 and hi - lo < pt.gran:
            hi = lo
        rows = rows_of_piece(start, lo, hi) if hi > lo else []
        w = [(b, b, b, max(int(start[b]), lo), min(int(start[b + 1]), hi)) for b in rows]
        if mutant == "cut_page_to_previous_row" and w and kind == "static" and i > 0 and pt.pieces[i - 1][2] == "static" \
                and lo == start[rows[0]] and live[:rows[0]].any():
            b, prev = rows[0], int(np.nonzero(live[:rows[0]])[0][-1])
            w = [(prev, prev, b, lo, lo + 1)] + ([(b, b, b, lo + 1, w[0][4])] if w[0][4] > lo + 1 else []) + w[1:]
        if mutant == "first_maxseg_rows_only":
            w = [x for x in w if x[0] < rows[0] + maxseg]
        if mutant == "empty_rows_shift_q":
            w = [(b, rows[0] + rows.index(b), b, a, z) for b, _, _, a, z in w]
        work.append(w)
    # what the contract says of every row: its pieces in page order, and how many triples its merge waits for
    met = {b: [] for b in np.nonzero(live)[0]}
    if mutant == "cut_page_to_previous_row":          # (a wrong row search is wrong everywhere: the counts follow it)
        for i, w in enumerate(work):
            for x in w:
                met[x[0]].append(i)
    else:
        for i, (lo, hi, kind) in enumerate(pt.pieces):
            for b in rows_of_piece(start, lo, hi):
                met[b].append(i)
    expected = {b: len(p) for b, p in met.items()}
    if mutant == "arrivals_one_too_many":
        static_cuts = {hi for lo, hi, kind in pt.pieces if kind == "static"}
        for b in expected:
            if int(start[b + 1]) in static_cuts:
                expected[b] += 1
    slots = {b: {} for b in met}
    arrived = {b: 0 for b in met}
    for i, w in enumerate(work):
        for dest, q_row, b, a, z in w:
            t = triple(q_row, b, (a - int(start[b])) * PAGE, min((z - int(start[b])) * PAGE, int(L[b])))
            if expected[dest] == 1:
                out[dest] = t[2] / t[1]
                continue
            slot = met[dest].index(i)
            if mutant == "granule_slot_on_last_static" and pt.pieces[i][2] == "granule" \
                    and any(pt.pieces[j][2] == "static" for j in met[dest]):
                slot -= 1
            slots[dest][slot] = t
            arrived[dest] += 1
            if arrived[dest] == expected[dest]:
                out[dest] = merged([slots[dest][k] for k in sorted(slots[dest])], rescale=mutant != "merge_without_rescale")
    return out


def vector_case(seed, lengths, S, D):
    """accuracy_cases.base_case for a length vector, with caches only as long as the longest row needs (one_page_rows
    is 2048 rows of at most 16 tokens: dense [B, S, D] caches would be 64 times what the rows hold).  The page table of
    the case is S_case / 16 wide; the kernels get it widened to S / 16 (tests/accuracy_gpu.py)."""
    from accuracy_cases import base_case
    L = np.asarray(lengths, np.int32)
    S_case = min(S, max(PAGE, -(-(int(L.max()) + 1) // PAGE) * PAGE))
    return base_case(seed, len(L), S_case, D, L)
