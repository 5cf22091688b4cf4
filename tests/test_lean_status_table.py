"""Every status the eight lean entry points with heads, a window, sinks or grouped K/V heads return before anything is
launched, held to a table recorded from the library before these entry points shared one router (lean_status_table.json):
mli_decode_scan_paged_{heads,window,sinks,gqa} ("scan") and mli_paged_attention_lean_{heads,window,sinks,gqa} ("lean", which
fill first).  No GPU: every device pointer is null and there is no workspace, so the domain below holds only calls that are
answered before a launch -- by construction, since this file also runs where a launch would reach a device:
  refused  shapes no scan takes (BAD_HEADS + BAD_PLAIN of test_window_abi.py), plain, windowed and with sinks, every divisor
           of n_heads as n_kv_heads; one head only under a window (without one it is the plain single-head scan's business);
  counts   head counts, sink counts, windows and element types outside an entry point's domain, at shapes that would
           otherwise launch: every call carries one such argument;
  accepted shapes the scans take, at n_batch 8 and n_sequence 1024, scan forms only: the default item is 64 tokens there and
           every window spans more (window >= 49), so every call has several items per row and no workspace to put them in.
A row is (entry point, form, n_batch, n_sequence, emb_dim, n_heads, n_kv_heads, window, n_sink, elem); an entry point is given
the rows its signature can express."""
import json
import os

from test_window_abi import BAD_HEADS, BAD_PLAIN

BAD_ARG, WORKSPACE, F32, BF16, FP8 = -22, -12, 0, 1, 2
TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lean_status_table.json")


def _divisors(n):
    return [d for d in range(1, n + 1) if n % d == 0]


def _kind_is_plain(S, W, K):          # lean_scan_kind (scan_plan.hpp)
    return W <= 0 or W >= S or (K > 0 and K + W >= S)


def _entries(H, Hkv, W, K):
    """the entry points whose signature can express (n_heads, n_kv_heads, window, n_sink)"""
    e = ["gqa"]
    if Hkv == H:
        e.append("sinks")
        if K == 0:
            e.append("window")
            if W == 0:
                e.append("heads")
    return e


def rows():
    """{key: (section, entry, form, B, S, D, H, Hkv, W, K, elem)}, in a fixed order"""
    out = {}

    def add(section, forms, B, S, D, H, Hkv, W, K, elem, only=None):
        for entry in _entries(H, Hkv, W, K):
            if only is not None and entry not in only:
                continue
            for form in forms:
                # one head without a window is mli_paged_attention_lean, which fills before it scans
                if form == "lean" and H == 1 and _kind_is_plain(S, W, K):
                    continue
                out[" ".join(map(str, (form, entry, B, S, D, H, Hkv, W, K, elem)))] = (section, entry, form, B, S, D, H, Hkv, W, K, elem)

    both = ("scan", "lean")
    for _, B, S, D, H, elem in BAD_HEADS + BAD_PLAIN:
        forms = [(12, 0), (12, 4), (1, 1), (S - 2, 1)] + ([(0, 0), (S, 0), (S - 4, 4)] if H > 1 else [])
        for Hkv in _divisors(H):
            for W, K in forms:
                # a window below one is another refusal (counts): only the entry point that reads it as "no window"
                add("refused", both, B, S, D, H, Hkv, W, K, elem, only=None if W >= 1 else ("gqa", "heads"))

    for S in (64, 16):
        B, D = 8, 128
        for H in (-2, 0):
            for elem in (F32, BF16, FP8):
                for W, K in ((0, 0), (12, 0), (12, 4)):
                    for Hkv in (1, H):
                        add("counts", both, B, S, D, H, Hkv, W, K, elem)
        for H, Hkv in ((1, -1), (1, 0), (1, 2), (2, -1), (2, 0), (2, 3), (4, -1), (4, 0), (4, 3), (4, 8)):
            for elem in (F32, BF16):
                for W, K in ((0, 0), (12, 4)):
                    add("counts", both, B, S, D, H, Hkv, W, K, elem)
        for H in (1, 2):
            for Hkv in _divisors(H):
                for elem in (F32, BF16, FP8):
                    for W in (0, 12, S):
                        add("counts", both, B, S, D, H, Hkv, W, -1, elem)                       # n_sink < 0
                    for W in (0, -1):
                        for K in (0, 4):
                            add("counts", both, B, S, D, H, Hkv, W, K, elem, only=("window", "sinks"))   # window < 1
                for W, K in ((0, 0), (12, 0), (12, 4), (S, 0), (S, 4)):
                    add("counts", both, B, S, D, H, Hkv, W, K, 3)                                # no such element type
                    # fp8 pages: no heads and no grouping; _window and _sinks take them with one head
                    add("counts", both, B, S, D, H, Hkv, W, K, FP8, only=("heads", "gqa") if H == 1 else None)

    for B, S, D in ((8, 1024, 128), (8, 1024, 256)):
        for H, kv in ((1, (1, 2)), (2, (1, 2, 3)), (4, (1, 2, 3, 4, 8))):
            for Hkv in kv:
                for W in (-1, 0, 64, 256, 1023, 1024, 5000):
                    for K in (0, 4, 768, 4000):
                        for elem in (F32, BF16, FP8):
                            add("accepted", ("scan",), B, S, D, H, Hkv, W, K, elem)
    return out


def call(mli, entry, form, B, S, D, H, Hkv, W, K, elem):
    args = {"heads": (H,), "window": (H, W), "sinks": (H, W, K), "gqa": (H, Hkv, W, K)}[entry]
    if form == "scan":
        return getattr(mli, "mli_decode_scan_paged_" + entry)(None, None, None, None, B, S, D, *args, elem, None, 0, None)
    return getattr(mli, "mli_paged_attention_lean_" + entry)(None, None, None, None, None, None, None, None, B, S, D, 0, *args,
                                                             elem, None, 0, None)


def _table():
    with open(TABLE) as f:
        return json.load(f)


def test_the_table_covers_the_domain_and_holds_refusals_only():
    table, domain = _table(), rows()
    assert set(table) == set(domain)                       # no enumerated call is missing, none is stale
    assert 2000 <= len(domain) <= 6000
    for key, (section, entry, form, *_rest) in domain.items():
        assert table[key] in (BAD_ARG, WORKSPACE), key    # anything else had reached a launch when it was recorded
        if form == "lean" or section != "accepted":
            assert table[key] == BAD_ARG, key              # the fill-first forms are asked only where nothing may be filled
    for entry in ("heads", "window", "sinks", "gqa"):
        for form in ("scan", "lean"):
            assert any(r[1] == entry and r[2] == form for r in domain.values()), (entry, form)
        assert any(r[1] == entry and table[k] == WORKSPACE for k, r in domain.items()), entry


def test_every_status_is_the_recorded_one(mli):
    table = _table()
    wrong = {}
    for key, (_section, *row) in rows().items():
        got = call(mli, *row)
        if got != table[key]:
            wrong[key] = (got, table[key])
    assert not wrong, "%d of %d differ (got, recorded): %s" % (len(wrong), len(table), sorted(wrong.items())[:20])
