"""CPU checks of tests/tower_ref.py and of uniir_clip_tower_layout: the stage references are wired like the model (float64 agreement
with the autograd of oracle.clip_oracle), the exported workspace plan is sound for every layout flag, every case of
tests/tower_cases.py reaches the path it names, and the comparer of tests/test_tower_stages_gpu.py flags every seeded wiring defect.
No GPU: the library is only asked for host arithmetic."""
import copy
import ctypes as C
import itertools

import pytest
import torch

import tower_cases as TC
import tower_ref as TR
from tower_cases import CASES

FAKE = lambda name: 0x1000          # noqa: E731  the queries below never touch device memory
F64_GATE = 1e-10


# ------------------------------------------------------------------------------------------------------ the reference's own wiring
def _oracle_grads(sp, wt, inp, demb, order):
    """embeddings and parameter gradients of sum(emb * demb) from the oracle's autograd in float64, items taken in `order`"""
    from oracle import clip_oracle as O
    sd, names = TC.oracle_state(sp, wt)
    cfg = TC.oracle_config(sp)
    idx = torch.tensor(order)
    emb = O.encode_text(sd, inp[idx], cfg) if sp.is_text else O.encode_image(sd, inp[idx], cfg)
    (emb * demb[idx]).sum().backward()
    grads = {}
    for ours, key in names.items():
        g = sd[key].grad
        grads[ours] = g.reshape(sp.W, -1) if ours == "conv" else g
    out = torch.empty_like(emb)
    out[idx] = emb.detach()
    return out, grads


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


@pytest.mark.parametrize("case", ["V1-pool0", "V1-pool1", "T1-dense-pool0", "T1-dense-pool1", "T1-packed-pool0", "T1-packed-pool1"])
def test_composed_reference_is_the_oracle_in_float64(case, monkeypatch):
    """compose(exact=True) -- the stage references chained with nothing rounded -- against the autograd of oracle.clip_oracle on the
    same float64 weights: embeddings and every parameter gradient.  The two share no code: the oracle is the model as published,
    differentiated by autograd; the composition is tower.hip's launch list with hand-written backward stages, the pooled last block
    and the packed rows included.  The oracle's LayerNorm helper casts to fp32 as upstream does; for this test it is replaced by the
    same F.layer_norm call without the cast.  Gate: 1e-10 relative to the tensor's largest element.  A second float64 evaluation of
    the oracle with the items in reverse order (other summation orders in every weight gradient) is asserted to sit below the same
    gate, measured at 1e-15 .. 1e-13: the gate is float64 round-off through two LayerNorm-conditioned blocks, and a wiring defect
    is seven orders above it."""
    import torch.nn.functional as Fn
    from oracle import clip_oracle as O
    monkeypatch.setattr(O, "layer_norm", lambda x, w, b, eps=1e-5: Fn.layer_norm(x, (x.shape[-1],), w, b, eps))
    sp = CASES[case]
    wt = TC.make_weights(sp, exact=True)
    tr = TR.compose(sp, wt, TC.trace_inputs(sp, exact=True), exact=True)
    inp = tr["input"].double() if not sp.is_text else tr["input"]
    emb, grads = _oracle_grads(sp, wt, inp, tr["demb"], list(range(sp.M)))
    emb2, grads2 = _oracle_grads(sp, wt, inp, tr["demb"], list(range(sp.M))[::-1])
    worst = {"emb": (_rel(tr["emb"], emb), _rel(emb2, emb))}
    for name in sp.params():
        got = tr["g." + name] - tr["g0." + name]
        worst[name] = (_rel(got, grads[name]), _rel(grads2[name], grads[name]))
    print(case, "worst composed-vs-oracle", max(v[0] for v in worst.values()), "oracle reorder", max(v[1] for v in worst.values()))
    bad = {k: v for k, v in worst.items() if not (v[0] < F64_GATE and v[1] < F64_GATE)}
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------------- the layout
def _layout(sp, save, stash_act=1, recompute=0):
    from uniir_amd import _lib
    lib = _lib.load()
    t, keep = TC.describe(sp, FAKE, stash_act=stash_act, recompute=recompute)
    live = sp.R if sp.lens else -1
    lay = _lib.clip_tower_layout(t, sp.M, live, save)
    if sp.lens:
        total = lib.uniir_clip_tower_workspace_bytes_packed(C.byref(t), sp.M, sp.R, save)
    else:
        total = lib.uniir_clip_tower_workspace_bytes(C.byref(t), sp.M, save)
    return lay, total


@pytest.mark.parametrize("case", sorted(CASES))
def test_layout_regions_are_aligned_inside_and_disjoint(case):
    """uniir_clip_tower_layout for save on / off, stash_act 0 / 1, recompute 0 / 1 (dense and packed, pool_last_block 0 / 1 / 2 are
    the cases): every region 256-B aligned, inside `total`, no two overlapping (the layer sets expanded; one shared set when
    lay_stride is 0), and `total` the workspace query's answer.  The forward / backward transient union of the header: everything
    from `tmp` on is transient, `g` comes first and a forward-only layout ends right behind it."""
    sp = CASES[case]
    for save, stash, rec in itertools.product((0, 1), (0, 1), (0, 1)):
        lay, total = _layout(sp, save, stash, rec)
        assert lay.total == total > 0, (save, stash, rec, lay.total, total)
        assert lay.rows == sp.R
        assert (lay.save, lay.pool_last, lay.stash_act, lay.recompute) == (save, int(sp.pooled), int(bool(save and (stash or rec))),
                                                                           int(bool(save and rec)))
        regs = sorted(TC.regions(sp, lay), key=lambda r: r[1])
        names = {r[0].split("[")[0] for r in regs}
        assert ("pl_q" in names) == sp.pooled and ("pl_dhq" in names) == bool(sp.pooled and save)
        assert ("patches" in names) == (not sp.is_text) and ("dconv" in names) == bool(save and not sp.is_text)
        assert ("df" in names) == bool(save) and ("o_f" in names) == bool(save) and ("o_g" in names) == bool(lay.stash_act)
        assert ("xs" in names) == bool(lay.recompute) and ("o_x" in names) == (not lay.recompute)
        assert (lay.lay_stride > 0) == bool(save and not rec)
        for name, off, nbytes in regs:
            assert off % 256 == 0 and off >= 0 and off + nbytes <= lay.total, (name, off, nbytes, lay.total)
        for (n0, o0, b0), (n1, o1, _) in zip(regs, regs[1:]):
            assert o0 + b0 <= o1, f"{n0} [{o0}, {o0 + b0}) overlaps {n1} at {o1} (save {save} stash {stash} recompute {rec})"
        assert lay.g == lay.tmp and all(o < lay.tmp for n, o, _ in regs if not n.startswith(("d", "pl_d", "g")))
        if not save:
            assert lay.total == lay.g + ((sp.R * 4 * sp.W * 2 + 255) & ~255)


def test_layout_of_pool_value_1_above_512_tokens_is_that_of_0_and_bad_arguments_are_refused():
    from uniir_amd import _lib
    lib = _lib.load()
    a, _ = _layout(CASES["V3-pool0"], 1)
    b, _ = _layout(CASES["V3-pool1"], 1)
    c, _ = _layout(CASES["V3-pool2"], 1)
    fields = [n for n, _ in _lib.ClipTowerLayout._fields_]
    assert all(getattr(a, n) == getattr(b, n) for n in fields)
    assert c.pool_last == 1 and c.total > a.total and a.pool_last == b.pool_last == 0
    t, keep = TC.describe(CASES["V1-pool0"], FAKE)
    lay = _lib.ClipTowerLayout()
    assert lib.uniir_clip_tower_layout(C.byref(t), 3, -1, 1, None) == -1
    assert lib.uniir_clip_tower_layout(C.byref(t), 3, 40, 1, C.byref(lay)) == -1           # packed rows of a vision tower
    assert lib.uniir_clip_tower_layout(C.byref(t), 3, -2, 1, C.byref(lay)) == -1
    t.width = 100
    assert lib.uniir_clip_tower_layout(C.byref(t), 3, -1, 1, C.byref(lay)) == -2
    tt, keep2 = TC.describe(CASES["T1-packed-pool0"], FAKE)
    assert lib.uniir_clip_tower_layout(C.byref(tt), 5, 4, 1, C.byref(lay)) == -2           # fewer live rows than items
    assert lib.uniir_clip_tower_layout(C.byref(tt), 5, 5 * 77 + 1, 1, C.byref(lay)) == -2


# ------------------------------------------------------------------------------------------------------------- every case's path
def _gemms(sp):
    """(what, M, N, K) of every uniir_gemm a training step of the case launches on ALL rows (forward, dgrad, wgrad)"""
    R, W = sp.R, sp.W
    out = [("in_proj", R, 3 * W, W), ("out_proj", R, W, W), ("c_fc", R, 4 * W, W), ("c_proj", R, W, 4 * W),
           ("c_proj dgrad", R, 4 * W, W), ("c_fc dgrad", R, W, 4 * W), ("out_proj dgrad", R, W, W), ("in_proj dgrad", R, W, 3 * W),
           ("c_proj wgrad", W, 4 * W, R), ("c_fc wgrad", 4 * W, W, R), ("out_proj wgrad", W, W, R), ("in_proj wgrad", 3 * W, W, R)]
    if not sp.is_text:
        out += [("conv", sp.M * sp.G, W, sp.kpad), ("conv wgrad", W, sp.kpad, sp.M * sp.G)]
    return out


def _tile(g):
    what, M, N, K = g
    return TR.gemm_tile(M, N, K, wgrad=what.endswith("wgrad"))


def _splits(N, K, rows):
    from uniir_amd import _lib
    return _lib.load().uniir_gemm_wgrad_splits(rows, -(-N // 256) * -(-K // 256))


def test_every_case_reaches_the_path_it_names():
    v1, v2, v3, t1, t2, t2p = (CASES[n] for n in ("V1-pool1", "V2-pool1", "V3-pool2", "T1-dense-pool1", "T2-dense-pool1", "T2-packed-pool1"))
    # V1: every GEMM on the 128-tile kernel; the pooled block's weight gradients reduce over K = 3 rows; R = 51
    assert v1.R == 51 and all(_tile(g) == 128 for g in _gemms(v1))
    assert v1.pooled and v1.M == 3 and TR.attention_family(v1) == "resident"
    # V2: the all-row GEMMs on the 256-tile kernels, the pair-tile attention backward, every block weight gradient at 2 slabs
    assert v2.R == 2167 and all(_tile(g) == 256 for g in _gemms(v2))          # (R % 64 != 0: the wgrads run head + tail)
    assert TR.attention_family(v2) == "pair-tile-bwd"
    assert [_splits(N, K, v2.R) for N, K in ((v2.W, 4 * v2.W), (4 * v2.W, v2.W), (v2.W, v2.W), (3 * v2.W, v2.W))] == [2, 2, 2, 2]
    assert v2.E % 8 == 0 and v2.E % 64 != 0          # the projection's N is no multiple of a tile
    # V3: streaming attention; value 1 falls back to the full block, value 2 pools (the one-query kernels of attention_one.hip)
    assert v3.T == 577 > TR.ATT_SEQ_MAX and TR.attention_family(v3) == "streaming"
    assert not CASES["V3-pool1"].pooled and v3.pooled
    # T1: one head, causal, dense and packed; EOT at the first possible position and at the last
    assert t1.H == 1 and TR.attention_family(t1) == "causal" and TR.attention_family(CASES["T1-packed-pool0"]) == "causal-packed"
    assert TC.T1_EOT[0] == 1 and TC.T1_EOT[-1] == t1.T - 1 and CASES["T1-packed-pool0"].R == sum(e + 1 for e in TC.T1_EOT)
    txt = TC.make_input(t1)
    assert txt.argmax(1).tolist() == list(TC.T1_EOT) and bool((txt[2, :31] == 0).any()) and int(txt[3, 1]) == int(txt[3, 2])
    # T2: 256-tile GEMMs and split-K on the dense rows; fewer live rows packed; the column-range weight gradient (lddy = 3W)
    assert t2.R == 2310 and all(_tile(g) == 256 for g in _gemms(t2))
    assert _splits(4 * t2.W, t2.W, t2.R) >= 2 and _splits(2 * t2.W, t2.W, t2.R) >= 2
    assert t2.M <= t2p.R < t2.R and min(t2p.lens) == 2 and max(t2p.lens) == t2.T
    assert TC.make_input(t2p).argmax(1).tolist() == list(TC.T2_EOT)


# -------------------------------------------------------------------------------------------------------------------- sensitivity
_COMPOSED = {}


def _composed(case):
    if case not in _COMPOSED:
        sp = CASES[case]
        wt = TC.make_weights(sp)
        _COMPOSED[case] = (wt, TR.compose(sp, wt, TC.trace_inputs(sp)))
    return _COMPOSED[case]


MUTATION_CASES = {True: ("V1-pool1", "T1-packed-pool1"), False: ("V1-pool0", "T1-dense-pool0"), None: ("V1-pool0", "T1-dense-pool1")}


@pytest.mark.parametrize("case", ["V1-pool0", "V1-pool1", "T1-dense-pool0", "T1-dense-pool1", "T1-packed-pool1"])
def test_composed_trace_passes_the_comparer(case):
    """the unmutated data: every stage output of compose() is its own reference rounded once to the stored type, so the comparer
    accepts all of it, and no stage is absent"""
    wt, tr = _composed(case)
    res = TR.verify(CASES[case], wt, tr)
    assert not TR.failures(res), TR.failures(res)[:5]
    assert len(res) > 40


@pytest.mark.parametrize("mutation", [m[0] for m in TR.MUTATIONS])
def test_comparer_flags_every_seeded_wiring_defect(mutation):
    """every defect of tower_ref.MUTATIONS, applied to a copy of the composed trace, is flagged by verify() -- the comparer the GPU
    test uses -- at each case it is listed for, and only stages that read or write the touched tensor object"""
    name, pooled, fn = next(m for m in TR.MUTATIONS if m[0] == mutation)
    for case in MUTATION_CASES[pooled]:
        sp = CASES[case]
        wt, clean = _composed(case)
        tr = copy.deepcopy(clean)
        fn(sp, wt, tr)
        bad = TR.failures(TR.verify(sp, wt, tr))
        print(case, mutation, "->", [(b[0], b[1]) for b in bad])
        assert bad, f"{mutation} at {case}: not seen by the comparer"
