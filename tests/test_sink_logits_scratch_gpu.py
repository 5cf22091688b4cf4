"""The four sink-logit entry points held to the scratch contract of include/mli_kernels.h with tests/scratch_fence.py, on fenced,
poisoned buffers -- the protocol and the helpers of tests/test_scratch_contract_gpu.py (imported, unchanged), the sink logits in
a fenced view of their own:
  - mli_decode_scan_paged_sink_logits: exactly mli_attention_heads_workspace_bytes is enough, the ladder of smaller sizes is
    refused without one byte of the arena changing, the guards stay intact, the counters end at zero, and the result is
    bit-identical with the workspace body zero, 0xFF and left behind by another call;
  - mli_paged_attention_lean_sink_logits: the same for fill -> latest -> scan, pages and q_output among the outputs;
  - mli_prompt_scan_paged_sink_logits: it has no scratch -- every guard around q, the segment arrays, the logits and the result
    stays intact and the rows of a skipped segment keep their sentinels;
  - mli_paged_prompt_logprobs_sink_logits: exactly mli_prompt_logprobs_scratch_bytes is enough, 256 bytes fewer answer
    MLI_ERR_WORKSPACE with nothing changed, and the outputs do not depend on what the scratch held.
Every result is judged by sink_logits_model's model and derived bound as well."""
import numpy as np
import pytest
import torch

import f64_model as fm
import prompt_model as pm
import scratch_fence as sf
import sink_logits_model as sl
from helpers import bf16_bits, paged_case
from test_scratch_contract_gpu import (ELEM, SENTINEL, WORKSPACE, Paged, _segment_arrays, carve_workspace, check_rows, contract,
                                       f32, heads_need, knobs, launches, length_vectors, nbytes_of, other_call, others,  # noqa: F401
                                       page_values, pages_on_device, place_all, place_pool, record_refusal, scan_case, stream)

pytestmark = pytest.mark.gpu


def _judge(q, ktm, v_rows, L, out, H, Hkv, z, W, K, what):
    model = sl.SinkLogitsModel(q, ktm, v_rows, L, H, Hkv, z, W, K)
    worst, tol = sl.compare(out, sl.eval_fp32(q, ktm, v_rows, L, H, Hkv, z, W, K), model, what=what)
    assert worst <= tol, f"{what}: {worst:.3e} > tol {tol:.3e}"


class SinkPaged(Paged):
    """Paged with the sink logits in the fenced view Paged keeps for a per-head float array"""

    def scan(self, mli, arena, p, entry, n, phases=7):
        if entry != "sink_logits":
            return super().scan(mli, arena, p, entry, n, phases)
        a = lambda name: arena.ptr(p + name)
        return mli.mli_decode_scan_paged_sink_logits(a("q"), a("table"), a("lengths"), a("out"), self.B, self.S, self.D, self.H,
                                                     self.Hkv, self.W, self.K, a("slopes"), ELEM[self.elem], arena.ptr("ws"), n,
                                                     stream())


@pytest.mark.parametrize("elem,H,Hkv,W,K", [(e, *f) for e in ("f32", "bf16") for f in ((2, 2, 0, 0), (2, 1, 40, 4), (2, 1, 100, 0))],
                         ids=lambda v: str(v))
def test_decode_scan(oracle, mli, dev, others, elem, H, Hkv, W, K):
    B, S, D = 12, 256, 128
    L = length_vectors(1400 + H + W, B, S)[0]
    pb = SinkPaged(oracle, dev, 1600 + 7 * H + W + K, B, S, D, elem, "mixed", L, H, Hkv, W, K, slopes=np.zeros(H, np.float32))
    pb.slopes = sl.learned(pb.q, pb.ktm, pb.L, H, Hkv, W, K)
    need = heads_need(mli, pb)
    what = f"decode_scan_paged_sink_logits {elem} ({B}, {S}, {D}) H {H} Hkv {Hkv} W {W} K {K}"
    with knobs(mli, chunk_tokens=64):
        assert mli.mli_launch_counts_reset() == 0
        _, out, _ = scan_case(mli, dev, pb, others["plain"], what, "sink_logits", need)
        assert launches(mli, "scan_heads_sink_logits") >= 4 and launches(mli, "scan_heads_window") == 0, f"{what}: another kernel"
    _judge(pb.q, pb.ktm, pb.v_rows, pb.L, out, H, Hkv, pb.slopes, W, K, what)


@pytest.mark.parametrize("elem,rope", [("f32", False), ("bf16", False), ("f32", True), ("bf16", True)])
def test_lean_composition(oracle, mli, dev, others, elem, rope):
    B, S, D, n_new, H, Hkv, W, K = 12, 256, 128, 3, 2, 1, 40, 4
    L = length_vectors(1900 + D, B, S)[0]
    c = paged_case(1951 + D, B, S, D, conditioned=True, lengths=L)
    new_idx = c["new_batch_idx"].copy()
    new_idx[:n_new] = [1, 2, 4]                                    # rows of 1, 63 and 65 tokens are new: filled from x
    pool, _ = pages_on_device(oracle, dev, c, c["q_output"], c["kt_cache"], c["v_cache"], elem, "nan")
    w = {k: c[k] if elem == "f32" else bf16_bits(c[k]).reshape(D, D) for k in ("wk", "wq", "wv")}
    z = np.asarray([0.5, -0.75], np.float32)
    need = int(mli.mli_attention_heads_workspace_bytes(B, S, D, H))
    other = others["plain"]
    n_other = heads_need(mli, other)
    inputs = {"wk": w["wk"], "wq": w["wq"], "wv": w["wv"], "new_idx": new_idx, "lengths": L, "z": z}
    if rope:
        import rope_model
        inputs["rope"] = rope_model.standard_table(S, D // H)
    outs = {"q": (B * D * 4, torch.float32, SENTINEL), "out": (B * D * 4, torch.float32, SENTINEL)}
    arena = sf.Arena(sf.Arena.room(*[nbytes_of(a) for a in inputs.values()], *[n for n, _, _ in outs.values()],
                                   nbytes_of(pool), c["table"].size * 8, *other.room(), max(need, n_other)), dev)
    place_all(arena, inputs, outs)
    place_pool(arena, pool, c["table"], elem)
    carve_workspace(arena, other, need, n_other)
    a = arena.ptr

    def call(n):
        return mli.mli_paged_attention_lean_sink_logits(a("table"), a("lengths"), a("wk"), a("wq"), a("wv"), a("new_idx"), a("q"),
                                                        a("out"), B, S, D, n_new, H, Hkv, W, K, a("z"), a("rope") if rope else None,
                                                        ELEM[elem], arena.ptr("ws"), n, stream())
    what = f"lean_sink_logits {elem} ({B}, {S}, {D}) H {H} Hkv {Hkv} W {W} K {K} rope {rope}"
    outputs = list(outs) + ["pool"]
    images = sf.save(arena, outputs)
    with knobs(mli, chunk_tokens=64):
        assert mli.mli_launch_counts_reset() == 0
        first = contract(arena, what, call, images, outputs, need, other=other_call(mli, arena, other, need))
        record_refusal(arena, what, call, need, images)
        assert launches(mli, "scan_heads_sink_logits") >= 3 and launches(mli, "scan_heads_window") == 0, f"{what}: another kernel"
    out, q = f32(first["out"], (B, D)), f32(first["q"], (B, D))
    check_rows(out, L, what)
    assert np.isfinite(q).all() and not (q[L > 0] == SENTINEL).any(), f"{what}: q_output"
    values = page_values(first["pool"], elem)
    k_rows, v_rows = fm.gather_pages(values, c["table"], L, S, D, 1), fm.gather_pages(values, c["table"], L, S, D, 2)
    _judge(q, np.ascontiguousarray(k_rows).transpose(0, 2, 1), v_rows, L, out, H, Hkv, z, W, K, what)


def _prompt_problem(oracle, dev, elem, H, seed):
    B, S, D, V = 4, 64, 128, 1030
    L = np.asarray([63, 40, 17, 33], np.int32)
    c = paged_case(seed, B, S, D, conditioned=True, lengths=L)
    pool, values = pages_on_device(oracle, dev, c, c["q_output"], c["kt_cache"], c["v_cache"], elem, "nan")
    # the third segment names row 7 of a batch of 4: skipped whole by every kernel of the call
    segs = [(2, 0, 17), (0, 50, 13), (7, 0, 4), (3, 5, 20), (0, 20, 9)]
    arrays, n = _segment_arrays(segs)
    skipped = np.zeros(n, bool)
    skipped[int(arrays[3][2]):int(arrays[3][2]) + 4] = True
    live = [s for s in segs if s[0] < B]
    rows, pos = pm.queries(live)
    ktm = fm.gather_pages(values, c["table"], L, S, D, 1).transpose(0, 2, 1)
    v_rows = fm.gather_pages(values, c["table"], L, S, D, 2)
    x_rows = fm.gather_pages(values, c["table"], L, S, D, 0)
    return B, S, D, V, L, c, pool, segs, arrays, n, skipped, rows, pos, ktm, v_rows, x_rows


@pytest.mark.parametrize("elem", ["f32", "bf16"])
def test_prompt_scan_has_no_scratch_and_stays_inside_its_arrays(oracle, mli, dev, elem):
    H, Hkv = 4, 2
    B, S, D, V, L, c, pool, segs, arrays, n, skipped, rows, pos, ktm, v_rows, x_rows = _prompt_problem(oracle, dev, elem, H, 2850)
    rng = np.random.default_rng(2851)
    qv = np.zeros((n, D), np.float32)
    qv[~skipped] = pm.query_vectors(c["q_output"], rows, pos)
    qv[skipped] = rng.standard_normal((int(skipped.sum()), D)).astype(np.float32)
    z = sl.learned(qv[~skipped], ktm[rows], pos + 1, H, Hkv)
    inputs = {"qv": qv, "z": z}
    inputs.update({f"seg{i}": a for i, a in enumerate(arrays)})
    outs = {"out": (n * D * 4, torch.float32, SENTINEL)}
    arena = sf.Arena(sf.Arena.room(*[nbytes_of(a) for a in inputs.values()], n * D * 4, nbytes_of(pool), c["table"].size * 8), dev)
    place_all(arena, inputs, outs)
    place_pool(arena, pool, c["table"], elem)
    a = arena.ptr
    what = f"prompt_scan_paged_sink_logits {elem} ({B}, {S}, {D}) H {H} Hkv {Hkv}"
    before = None
    for run in range(2):
        arena.view("out", torch.float32).fill_(SENTINEL)
        snap = arena.snapshot()
        assert mli.mli_launch_counts_reset() == 0
        rc = mli.mli_prompt_scan_paged_sink_logits(a("qv"), a("table"), a("seg0"), a("seg1"), a("seg2"), a("seg3"), a("out"), len(segs),
                                                   20, n, B, S, D, H, Hkv, 0, 0, a("z"), ELEM[elem], stream())
        torch.cuda.synchronize()
        assert rc == 0 and launches(mli, "scan_prompt_sink_logits") == 1 and launches(mli, "scan_prompt") == 0, (what, rc)
        arena.assert_guards_intact(what)
        got = sf.bits(arena.view("out"))
        if before is not None:
            sf.assert_same_bits(got, before, f"{what}: second launch")
        before = got
        # a refusal changes nothing: no logits
        arena.view("out", torch.float32).fill_(SENTINEL)
        snap = arena.snapshot()
        rc = mli.mli_prompt_scan_paged_sink_logits(a("qv"), a("table"), a("seg0"), a("seg1"), a("seg2"), a("seg3"), a("out"), len(segs),
                                                   20, n, B, S, D, H, Hkv, 0, 0, None, ELEM[elem], stream())
        torch.cuda.synchronize()
        assert rc == -22
        arena.assert_unchanged(snap, f"{what}: refused")
    out = f32(before, (n, D))
    assert (out[skipped] == SENTINEL).all(), f"{what}: a skipped segment's rows were written"
    assert np.isfinite(out).all() and not (out[~skipped] == SENTINEL).any(), what
    model = sl.prompt_model(qv[~skipped], ktm, v_rows, rows, pos, H, Hkv, z)
    worst, tol = sl.compare(out[~skipped], sl.prompt_eval_fp32(qv[~skipped], ktm, v_rows, rows, pos, H, Hkv, z), model, what=what)
    assert worst <= tol


@pytest.mark.parametrize("elem,n_top", [("f32", 0), ("f32", 8), ("bf16", 0), ("bf16", 8)])
def test_paged_prompt_logprobs(oracle, mli, dev, elem, n_top):
    import gemm_model as gm
    from test_scratch_contract_gpu import ISENTINEL
    H, Hkv = 4, 2
    B, S, D, V, L, c, pool, segs, arrays, n, skipped, rows, pos, ktm, v_rows, x_rows = _prompt_problem(oracle, dev, elem, H, 2860)
    rng = np.random.default_rng(2861 + H)
    emb = (rng.standard_normal((V, D)) * 0.5).astype(np.float32)
    inp = rng.integers(0, V, size=(B, S)).astype(np.int32)
    w32 = (rng.standard_normal((D, D)) * (2.0 / np.sqrt(D))).astype(np.float32)
    wq = w32 if elem == "f32" else bf16_bits(w32).reshape(D, D)
    w_values = gm.decode(wq, "f32" if elem == "f32" else "bf16").astype(np.float64)
    z = np.asarray([1.0, -0.5, 0.25, 2.0], np.float32)
    other_segs = [(1, 3, 30), (3, 0, 2)]
    o_arrays, o_n = _segment_arrays(other_segs)
    V_other = 515
    need = int(mli.mli_prompt_logprobs_scratch_bytes(n, D, V))
    n_other = int(mli.mli_prompt_logprobs_scratch_bytes(o_n, D, V_other))
    assert 0 < n_other < need
    inputs = {"inp": inp, "wq": wq, "emb": emb, "z": z}
    inputs.update({f"seg{i}": a for i, a in enumerate(arrays)})
    inputs.update({f"o.seg{i}": a for i, a in enumerate(o_arrays)})
    outs = {"lp": (n * 4, torch.float32, SENTINEL), "o.lp": (o_n * 4, torch.float32, SENTINEL)}
    if n_top:
        outs.update({"ids": (n * n_top * 4, torch.int32, ISENTINEL), "tops": (n * n_top * 4, torch.float32, SENTINEL)})
    arena = sf.Arena(sf.Arena.room(*[nbytes_of(a) for a in inputs.values()], *[b for b, _, _ in outs.values()], nbytes_of(pool),
                                   c["table"].size * 8, need), dev)
    place_all(arena, inputs, outs)
    place_pool(arena, pool, c["table"], elem)
    arena.carve("ws", need)
    a = arena.ptr

    def run(p, lp, n_pos, vocab, top, count, n_seg, scratch_bytes, sunk):
        front = (a("table"), a("inp"), a("wq"), a("emb"), a(p + "seg0"), a(p + "seg1"), a(p + "seg2"), a(p + "seg3"), a(lp),
                 a("ids") if top else None, a("tops") if top else None)
        shape = (n_seg, count, n_pos, B, S, D, vocab, H, Hkv, 0, 0)
        tail = (ELEM[elem], top, arena.ptr("ws"), scratch_bytes, stream())
        if sunk:
            return mli.mli_paged_prompt_logprobs_sink_logits(*front, *shape, a("z"), *tail)
        return mli.mli_paged_prompt_logprobs(*front, *shape, *tail)

    def call(nbytes):
        return run("", "lp", n, V, n_top, 20, len(segs), nbytes, True)

    def other():
        arena.resize("ws", n_other)
        rc = run("o.", "o.lp", o_n, V_other, 0, 30, len(other_segs), n_other, False)
        arena.assert_guards_intact("the other call")
        arena.resize("ws", need)
        return rc

    what = f"paged_prompt_logprobs_sink_logits {elem} ({B}, {S}, {D}, {V}) H {H} Hkv {Hkv} n_top {n_top}"
    outputs = [k for k in outs if not k.startswith("o.")]
    images = sf.save(arena, outputs)
    assert mli.mli_launch_counts_reset() == 0
    first = contract(arena, what, call, images, outputs, need, other=other, counters=0)
    assert launches(mli, "scan_prompt_sink_logits") == 3 and launches(mli, "scan_prompt") == 1, f"{what}: three calls and the other one"
    rungs = sf.run_ladder(arena, "ws", [need - 256, need], call, images, outputs, first, 0, what)
    assert rungs == [(need - 256, WORKSPACE), (need, 0)], rungs
    lp = f32(first["lp"], (n,))
    assert (lp[skipped] == SENTINEL).all(), f"{what}: token_logprob of a skipped segment was written"
    ids = tops = np.zeros((n, 0))
    if n_top:
        ids, tops = first["ids"].view(np.int32).reshape(n, n_top), f32(first["tops"], (n, n_top))
        assert (ids[skipped] == ISENTINEL).all() and (tops[skipped] == SENTINEL).all(), f"{what}: top_* of a skipped segment"
    q64 = x_rows.astype(np.float64)[rows, pos] @ w_values
    attn = sl.prompt_model(q64, ktm, v_rows, rows, pos, H, Hkv, z).o
    logits = (attn @ emb.astype(np.float64).T).astype(np.float32)
    given = np.asarray([inp[r, t + 1] if t + 1 < S else -1 for r, t in zip(rows, pos)], np.int64)
    err, tol, bad = pm.compare_given((lp[~skipped], ids[~skipped], tops[~skipped]), logits, given, n_top)
    print(f"SCRATCH {what} | figures: error {err:.3e}  tolerance {tol:.3e}")
    assert not bad and err <= tol, (what, err, tol, bad)
