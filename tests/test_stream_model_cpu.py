"""Proves on the CPU what tests/test_stream_partition_gpu.py relies on: that the named length vectors of
tests/stream_model.py reach every partition event of the equal-page-shares scan on chips of 256, 304 and 104 CUs, that
the restated partition evaluated piece by piece IS the float64 model, and that the project's comparison -- its metric, its
tolerance from the fp32 oracle's own error -- fails for nine partition bugs by at least 4x, on the vectors the tables
below name.  The tables are asserted: a vector that is dropped, or a tolerance that is widened, fails here without a GPU."""
import functools

import numpy as np
import pytest

import f64_model as fm
import stream_model as sm
from accuracy_cases import apply_family, oracle_scan

S = 1024
G_LAUNCHES = (512, 608, 208)      # 2 x CUs: MI355X / MI300X-class 304 / a 104-CU part
GAP = 4.0

# What every named vector must ADD to the vectors before it, whatever the chip (union over sm.SPLITS).  A vector that adds
# nothing does not belong in the list.  Reasoned from the construction and confirmed by running events():
#   one_row_per_share    16-page rows against 16-page shares: with static shares only every cut is a row start and every
#                        row whole; the dynamic splits move Ps off the grid -- rows in 2 pieces, static + granule triples,
#                        64- and 256-page granules over 4 and 16 rows, a short last granule
#   shifted_by_one_page  P = 16 G_launch - 1: one workgroup fewer, shares a little over 16 pages, so the cuts drift through
#                        the rows one page at a time; at 60 % the 6-page shares cut a row into 4 and more
#   full_rows            2048 pages in 128 shares of 16: every row is exactly 4 whole shares
#   full_rows_to_S       ... with L == S
#   one_page_rows        every page is a row start, so every granule starts on one; 16 rows and more per piece
#   sparse               six empty rows between two live ones, inside the pieces; row 0 and the last row empty
#   tiny                 P = 0, and P < 32: one workgroup
ADDS = {
    "one_row_per_share": {"dynamic_on", "static_cut_on_row_start", "row_whole", "row_in_2_pieces", "row_static_and_dynamic",
                          "granule_straddles_rows", "last_granule_short", "more_rows_than_maxseg"},
    "shifted_by_one_page": {"fewer_workgroups", "row_in_4_or_more_pieces"},
    "full_rows": {"row_is_whole_shares"},
    "full_rows_to_S": {"row_of_length_S"},
    "one_page_rows": {"granule_cut_on_row_start"},
    "sparse": {"empty_row_in_piece", "empty_run_over_maxseg", "leading_empty_row", "trailing_empty_row"},
    "tiny": {"no_pages", "one_workgroup"},
}
# ... and the two that some vector reaches on every chip, but not the same vector on each
SOMEWHERE = {"dynamic_too_small", "piece_under_4_pages"}


def _events(lengths, G_launch):
    ev = set()
    for dyn, gran in sm.SPLITS:
        ev |= sm.events(lengths, S, G_launch, dyn, gran)
    return ev


@pytest.mark.parametrize("G_launch", G_LAUNCHES)
def test_the_vectors_reach_every_partition_event(G_launch):
    vectors = sm.stream_vectors(G_launch, S)
    assert list(vectors) == list(ADDS), "the table above names every vector, in order"
    assert set().union(*ADDS.values()) | SOMEWHERE == set(sm.EVENTS)
    seen = set()
    for name, group in vectors.items():
        ev = set().union(*(_events(L, G_launch) for L in group))
        new = ev - seen
        print(f"{name:20s} adds {sorted(new)}")
        assert new, f"{name} reaches nothing the vectors before it do not: delete it"
        assert ADDS[name] <= new, f"{name}: expected to add {sorted(ADDS[name] - new)} as well"
        seen |= ev
    assert seen == set(sm.EVENTS), sorted(set(sm.EVENTS) - seen)
    # MAXSEG = 2 (the kernels of 1024-wide rows): the group events still hold
    ev2 = set().union(*(sm.events(L, S, G_launch, d, g, maxseg=2) for grp in vectors.values() for L in grp for d, g in sm.SPLITS))
    assert {"more_rows_than_maxseg", "empty_run_over_maxseg"} <= ev2


def test_partition_of_a_vector_worked_by_hand():
    """full_rows at G_launch = 512, static shares only: P = 2048, G = 128 (P // 16), every share 16 pages, every row 4;
    at 4 % in 64-page granules: 81 dynamic pages = one granule of 64 and one of 17, Ps = 1967."""
    L = sm.stream_vectors(512, S)["full_rows"][0]
    pt = sm.partition(L, S, 512, 0, 64)
    assert (pt.P, pt.G, pt.Ps, pt.n_gran) == (2048, 128, 2048, 0)
    assert pt.pieces == [(16 * w, 16 * w + 16, "static") for w in range(128)] and (pt.row_pieces == 4).all()
    pt = sm.partition(L, S, 512, 4, 64)
    assert (pt.P, pt.G, pt.Ps, pt.n_gran) == (2048, 128, 1967, 2)
    assert pt.pieces[-2:] == [(1967, 2031, "granule"), (2031, 2048, "granule")]
    assert pt.row_pieces[31] == 2           # pages 1984 .. 2047: both granules and nothing else
    assert pt.row_pieces[30] == 3 + 1       # pages 1920 .. 1983: shares 125 (from 125 * 1967 // 128 = 1920), 126, 127; granule 0
    assert sum(hi - lo for lo, hi, _ in pt.pieces) == pt.P
    pt = sm.partition([5, 0, 17], S, 512, 12, 16)
    assert (pt.P, pt.G, pt.Ps, pt.n_gran, pt.pieces) == (3, 1, 3, 0, [(0, 3, "static")]) and pt.row_pieces.tolist() == [1, 0, 1]
    assert sm.partition([0, 0], S, 512, 4, 64).pieces == []


# Which vectors see which wrong variant, in `flat` at D = 64 and G_launch = 512, under at least one split: the worst row is
# off by at least 4x the case's tolerance.  Reasoned from what each variant needs, confirmed by running the float64 model:
#   share_drops_last_page        every vector with a page
#   cut_page_to_previous_row     needs a cut between two static shares on a row start: every vector has one under some
#                                split (tiny: [256, 255], P = 32 in two shares)
#   arrivals_one_too_many        needs a row that ends on a cut, and the last share always ends on one
#   granule_slot_on_last_static  needs a row with static and dynamic triples: no one-page row has both
#   last_granule_skipped         needs a dynamic part whose size is no multiple of the granule
#   first_maxseg_rows_only       needs more than 4 rows in a piece: not full_rows (64-page rows)
#   empty_rows_shift_q           needs an empty row inside a piece: sparse, and tiny's [5, 0, 17]
#   merge_without_rescale        needs a row in 2 pieces
#   length_S_as_S_minus_1        needs a row of S tokens
EVERY = {"one_row_per_share", "shifted_by_one_page", "full_rows", "full_rows_to_S", "one_page_rows", "sparse", "tiny"}
SEES = {
    "share_drops_last_page": EVERY,
    "cut_page_to_previous_row": EVERY,
    "arrivals_one_too_many": EVERY,
    "granule_slot_on_last_static": EVERY - {"one_page_rows"},
    "last_granule_skipped": EVERY,
    "first_maxseg_rows_only": EVERY - {"full_rows", "full_rows_to_S", "tiny"},
    "empty_rows_shift_q": {"sparse", "tiny"},
    "merge_without_rescale": EVERY - {"one_page_rows"},
    "length_S_as_S_minus_1": {"full_rows_to_S"},
}
PEAK_VECTORS = set(sm.PEAK_VECTORS)


@functools.lru_cache(maxsize=None)
def _measure(oracle, name, family, G_launch=512, D=64):
    """{variant: worst row's error / tolerance over the vector's arrays and the splits}, and the same for the oracle and for
    the unmodified restatement (against the model: an absolute difference)."""
    worst = {mu: 0.0 for mu in sm.MUTANTS}
    e_oracle, restated = 0.0, 0.0
    for k, L in enumerate(sm.stream_vectors(G_launch, S)[name]):
        c = sm.vector_case(7200 + k, L, S, D)
        q, kt = apply_family(c, family)
        v = c["v_cache"]
        m = fm.Model(q, kt, v, L)
        e = fm.attention_error(oracle_scan(oracle, q, kt, v, L)[2], m)
        tol = fm.tolerance(e)
        e_oracle = max(e_oracle, float(e.max()) / tol)
        cache = {}
        for dyn, gran in sm.SPLITS:
            pt = sm.partition(L, S, G_launch, dyn, gran)
            restated = max(restated, float(np.abs(sm.piecewise_attention(q, kt, v, L, pt, cache=cache) - m.o).max()))
            for mu in sm.MUTANTS:
                with np.errstate(all="ignore"):
                    got = sm.piecewise_attention(q, kt, v, L, pt, mutant=mu, cache=cache)
                worst[mu] = max(worst[mu], float(fm.attention_error(got, m).max()) / tol)
    return worst, e_oracle, restated


@pytest.mark.parametrize("name", list(ADDS))
def test_the_restatement_is_the_model_and_the_comparison_bites(oracle, name):
    worst, e_oracle, restated = _measure(oracle, name, "flat")
    print(f"{name}: oracle / tol {e_oracle:.2f}  restatement - model {restated:.1e}  variant / tol: " +
          " ".join(f"{mu}={w:.1e}" for mu, w in worst.items()))
    assert restated <= 1e-12, "piecewise_attention without a variant is the float64 model"
    assert e_oracle <= 1.0, "the oracle passes its own tolerance"
    for mu, vectors in SEES.items():
        if name in vectors:
            assert worst[mu] >= GAP, f"{mu} was expected to show on {name}: {worst[mu]:.2e} x tol"
        else:
            assert worst[mu] <= 1.0, f"{mu} was expected to change nothing on {name}: {worst[mu]:.2e} x tol"


def test_every_variant_is_seen_by_some_vector():
    assert set(SEES) == set(sm.MUTANTS) and all(SEES.values())
    assert all(v <= set(ADDS) for v in SEES.values())


@pytest.mark.parametrize("family", ["early_peak", "late_peak"])
@pytest.mark.parametrize("name", sorted(PEAK_VECTORS))
def test_a_merge_without_rescaling_shows_in_the_peak_families(oracle, name, family):
    """Where one piece of a row holds tokens that carry e^30 the weight of the others, a merge that forgets exp(m_i - m)
    gives the other pieces e^30 too much: the families the GPU test adds on the vectors with rows in two or more pieces."""
    assert any((sm.partition(L, S, 512, d, g).row_pieces >= 2).any() for L in sm.stream_vectors(512, S)[name] for d, g in sm.SPLITS)
    worst, e_oracle, restated = _measure(oracle, name, family)
    assert restated <= 1e-12 and e_oracle <= 1.0
    assert worst["merge_without_rescale"] >= GAP, worst["merge_without_rescale"]


@pytest.mark.parametrize("G_launch", G_LAUNCHES)
def test_the_layout_of_the_gpu_test_follows_the_vectors(G_launch):
    """early_peak / late_peak go to the vectors with a row in two or more pieces, the wide-row kernels to those of at most
    2048 pages: the GPU test lists them by name (it is laid out before a device is there)."""
    vectors = sm.stream_vectors(G_launch, S)
    assert {n: len(g) for n, g in vectors.items()} == sm.N_ARRAYS
    split_rows = {n for n, g in vectors.items() if any((sm.partition(L, S, G_launch, d, gr).row_pieces >= 2).any()
                                                       for L in g for d, gr in sm.SPLITS)}
    assert split_rows == set(sm.PEAK_VECTORS) == EVERY - {"one_page_rows"}
    assert {n for n, g in vectors.items() if all(sm.page_counts(L, S).sum() <= 2048 for L in g)} == set(sm.SMALL_VECTORS)
    assert set(sm.OFFSET_VECTORS) <= set(vectors)


def test_a_row_of_S_tokens_cut_to_S_minus_1_fails_on_every_such_row(oracle):
    """One token in 1024 of a flat row moves the result by ~ 1 / 1024 of |v - o| ~ 1e-3 of the row's scale; fp32 rounding of a
    1024-term sum is ~ 1e-7 and the tolerance eight times that.  So the variant must fail by far more than the 4x that is
    asked of every variant: three orders of magnitude lie between one token and the tolerance, and at least 400x is held
    here -- which a tolerance ten times wider does not pass."""
    L = sm.stream_vectors(512, S)["full_rows_to_S"][0]
    assert (L == S).sum() == 4 and (L == S - 1).sum() == 28
    c = sm.vector_case(7200, L, S, 64)
    q, kt = apply_family(c, "flat")
    m = fm.Model(q, kt, c["v_cache"], L)
    tol = fm.tolerance(fm.attention_error(oracle_scan(oracle, q, kt, c["v_cache"], L)[2], m))
    pt = sm.partition(L, S, 512, 4, 64)
    err = fm.attention_error(sm.piecewise_attention(q, kt, c["v_cache"], L, pt, mutant="length_S_as_S_minus_1"), m)
    print(f"tol {tol:.2e}; rows of S tokens off by {err[L == S] / tol} x tol")
    assert (err[L == S] >= 400 * tol).all() and (err[L < S] <= tol).all()
