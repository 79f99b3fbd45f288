"""uniir_attention_rel_fwd_long / _rel_bwd_long -- T5-style self-attention (scale 1, bucketed relative bias, probability dropout) for
1 <= seq <= 1024 on the streaming kernels attn_rlong_* of csrc/attention_long.hip -- against the fp64 reference of
tests/attention_ref.py, element by element, with the machinery and the requirements of tests/test_attention_paths_gpu.py:
  every output of every item inside its bound; every tensor has a NaN guard band and everything outside the logical extent comes back
  bit for bit; forward and backward run twice and are compared with torch.equal -- drel included: the calls go through the stream of
  uniir_amd.ops, which has scratch registered, so the partials of (item, key block) are added in a fixed order; the backward runs on
  the rounded REFERENCE out / lse and, for `chained` cases, once more on the kernel's own forward.  One OBS line per case holds the
  largest |got - ref| / bound of every output.
drel is judged against attention_rel_long_ref.drel_call_bound: the reference's per-item bounds plus the fp32 error of adding batch *
ceil(seq / 128) + 2 partials plus the fixed-point quantum, 2^-41 per element of the bucket.
The case table (tests/attention_rel_long_cases.py) is checked on the CPU by tests/test_attention_rel_long_ref.py.
Further: drel accumulates; the calls the entry points refuse on the host; the new entry points at 334 and 512 tokens against
uniir_attention_rel_fwd / _rel_bwd (same bounds; whether the bits agree is printed, not asserted); a backward without enough scratch is
counted by uniir_reduce_stats and still inside the bound; the older entry points still stop at 512."""
import ctypes as C
import faulthandler

import pytest
import torch

import attention_ref as R
import attention_rel_long_ref as RL
from attention_ref import Case
from attention_rel_long_cases import CASES, NAMES
from test_attention_paths_gpu import (DEV, DROP_SEED, ERR, TAIL, Buf, Run, _bwd_refs, _dropf, _fmt, _judge, _lib, _round_ref, _stream,
                                      _untouched)

pytestmark = pytest.mark.gpu
CASE_SECONDS = 120    # a case takes a few seconds; a hung kernel ends the run here instead of at the runner's limit
BF = torch.bfloat16


class RunRelLong(Run):
    """the buffers of Run (api "rel": one packed qkv buffer), the calls of the new entry points.  drel_init: what drel holds before
    the backward (None: zeros); stream: the handle the backward is launched on (None: the stream of uniir_amd.ops)"""

    def forward(self):
        c, lib, W = self.c, _lib(), self.W
        self.out = Buf(self.nq, W, self.out_ld, c.dtype)
        self.lse = Buf(1, c.batch * c.heads * c.tq, c.batch * c.heads * c.tq + TAIL, torch.float32)
        before = {"out": self.out.bits().clone(), "lse": self.lse.bits().clone()}
        it = self.items[0]
        self.emb, self.bucket = it.rel_emb.contiguous(), it.rel_bucket.contiguous()
        rc = lib.uniir_attention_rel_fwd_long(self.X.ptr(0), self.out.ptr(), self.lse.ptr(), C.c_void_p(self.emb.data_ptr()),
                                              C.c_void_p(self.bucket.data_ptr()), c.nbuckets, 1.0, c.batch, c.tq, c.heads, c.drop_p,
                                              DROP_SEED, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        _untouched(f"{c.name} out", self.out, before["out"])
        _untouched(f"{c.name} lse", self.lse, before["lse"])
        return self.item_outputs_fwd()

    def backward(self, out_in, lse_in, dout=None, drel_init=None, stream=None):
        c, lib, W = self.c, _lib(), self.W
        O, dO = Buf(self.nq, W, self.out_ld, c.dtype), Buf(self.nq, W, self.out_ld, c.dtype)
        L = Buf(1, c.batch * c.heads * c.tq, c.batch * c.heads * c.tq + TAIL, torch.float32)
        lview = L.view[0].view(c.batch, c.heads, c.tq)
        for m, it in enumerate(self.items):
            O.view[self.q0[m]:self.q0[m] + c.tq] = out_in[m].reshape(c.tq, W)
            dO.view[self.q0[m]:self.q0[m] + c.tq] = (it.twin[3] if dout is None else dout[m]).reshape(c.tq, W)
            lview[m] = lse_in[m]
        self.dX = Buf(self.nq, 3 * W, 3 * W, c.dtype)
        self.drel = Buf(1, c.nbuckets * c.heads, c.nbuckets * c.heads + TAIL, torch.float32)
        if drel_init is None:
            self.drel.view.zero_()
        else:
            self.drel.view[0] = drel_init.flatten()
        outs = {"dqkv": self.dX, "drel": self.drel}
        before = {k: b.bits().clone() for k, b in outs.items()}
        rc = lib.uniir_attention_rel_bwd_long(self.X.ptr(0), O.ptr(), dO.ptr(), L.ptr(), self.dX.ptr(0), C.c_void_p(self.emb.data_ptr()),
                                              C.c_void_p(self.bucket.data_ptr()), c.nbuckets, 1.0, self.drel.ptr(), c.batch, c.tq,
                                              c.heads, c.drop_p, DROP_SEED, _stream() if stream is None else stream)
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        for name, b in outs.items():
            _untouched(f"{c.name} {name}", b, before[name])
        return self.item_outputs_bwd()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


_counts = {}


def _drel_judge(c, run, items, refs, ratios, what, init=None):
    key = (c.tq, c.nbuckets)
    if key not in _counts:
        _counts[key] = RL.bucket_counts(items[0])
    ref, bound = RL.drel_call_bound(refs, c.batch, c.tq, _counts[key])
    if init is not None:          # one more fp32 addition: into what drel held
        ref = ref + init.double()
        bound = bound + 2.0 * R.EPS32 * (init.double().abs() + ref.abs())
    got = run.drel.view[0].view(c.nbuckets, c.heads)
    why = R.compare(got, ref, bound, torch.float32)
    ratios["drel"] = max(ratios.get("drel", 0.0), R.worst(got, ref, bound))
    assert why is None, f"{c.name} ({c.path}) {what} drel: {why}"


def _forward_twice(c, run, items, ratios, what="forward"):
    got_f = run.forward()
    fref = [it.fwd_ref()[0] for it in items]
    _judge(c, what, got_f, fref, ratios)
    out_bits, lse_bits = run.out.bits().clone(), run.lse.bits().clone()
    own = [{k: v.clone() for k, v in g.items()} for g in got_f]
    run.forward()
    assert torch.equal(run.out.bits(), out_bits) and torch.equal(run.lse.bits(), lse_bits), f"{c.name}: the forward differs between two runs"
    return own, fref


def _backward_twice(c, run, items, what, o_in, l_in, ratios):
    from uniir_amd import ops
    got_b = run.backward(o_in, l_in)
    refs, dref = _bwd_refs(items, o_in, l_in)
    _judge(c, what, got_b, dref, ratios)
    _drel_judge(c, run, items, refs, ratios, what)
    bits = run.dX.bits().clone(), run.drel.bits().clone()
    ops.reset_reduce_stats()
    run.backward(o_in, l_in)
    assert ops.reduce_stats()[0] == 0, f"{c.name}: the {what} fell back to atomics with scratch registered: {ops.reduce_stats()}"
    assert torch.equal(run.dX.bits(), bits[0]), f"{c.name}: dqkv of the {what} differs between two runs"
    assert torch.equal(run.drel.bits(), bits[1]), f"{c.name}: drel of the {what} differs between two runs"
    return refs


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_attention_rel_long_path(case):
    c = case
    items = R.build_items(c, DEV, _dropf(c.drop_p) if c.drop_p > 0 else None)
    run = RunRelLong(c, items)
    ratios = {}
    own, fref = _forward_twice(c, run, items, ratios)
    print(f"\nOBS {c.name} [{c.path}] forward {_fmt(ratios)}")
    out_in, lse_in = _round_ref(c, fref)
    for what, (o_in, l_in) in (("backward", (out_in, lse_in)), ("chained", ([g["out"] for g in own], [g["lse"] for g in own]))):
        if what == "chained" and not c.chained:
            continue
        ratios = {}
        _backward_twice(c, run, items, what, o_in, l_in, ratios)
        print(f"OBS {c.name} [{c.path}] {what} {_fmt(ratios)}")


def test_drel_accumulates():
    """a second call into a drel that is not zero adds to it (the layers of a T5 stack share one table)"""
    c = Case("rel-long-129-accumulate", "attn_rlong_dkdv_kernel<0>", "rel", 2, 2, 129, nbuckets=32)
    items = R.build_items(c, DEV)
    run = RunRelLong(c, items)
    run.forward()
    out_in, lse_in = _round_ref(c, [it.fwd_ref()[0] for it in items])
    refs, _ = _bwd_refs(items, out_in, lse_in)
    init = torch.randn(c.nbuckets, c.heads, generator=torch.Generator().manual_seed(5)).to(DEV) * 3.0
    run.backward(out_in, lse_in, drel_init=init)
    ratios = {}
    _drel_judge(c, run, items, refs, ratios, "accumulate", init=init)
    once = run.drel.view[0].clone()
    run.backward(out_in, lse_in)
    fresh = run.drel.view[0].clone()
    # the partials' sum is the same bits in both calls (fixed order); the add into drel rounds once
    want = init.flatten().double() + fresh.double()
    assert bool(((once.double() - want).abs() <= R.EPS32 * want.abs()).all()), float((once.double() - want).abs().max())
    assert not torch.equal(once, fresh)
    print(f"\nOBS rel-long-129-accumulate {_fmt(ratios)}")


@pytest.mark.parametrize("seq", (334, 512))
def test_both_forms_fit_the_same_bounds_where_both_run(seq):
    """2 items, 2 heads, dropout 0.1: the streaming entry points and uniir_attention_rel_fwd / _rel_bwd on the same buffers, both inside
    the same bounds (the older form's drel with the bound tests/test_attention_paths_gpu.py holds it to, which is part of the new one).
    Whether the bits agree is an observation."""
    c = Case(f"rel-both-{seq}", "attn_fwd_kernel<1,1,0> + attn_bwd_kernel<1,1,0,512> | attn_rlong_*<1>", "rel", 2, 2, seq, drop_p=0.1,
             nbuckets=32)
    items = R.build_items(c, DEV, _dropf(c.drop_p))
    old, new = Run(c, items), RunRelLong(c, items)
    fref = [it.fwd_ref()[0] for it in items]
    out_in, lse_in = _round_ref(c, fref)
    refs, dref = _bwd_refs(items, out_in, lse_in)
    res = {}
    for name, run in (("resident", old), ("streamed", new)):
        ratios = {}
        _judge(c, f"{name} forward", run.forward(), fref, ratios)
        _judge(c, f"{name} backward", run.backward(out_in, lse_in), dref, ratios)
        _drel_judge(c, run, items, refs, ratios, f"{name} backward")
        res[name] = (run.out.bits().clone(), run.lse.bits().clone(), run.dX.bits().clone(), run.drel.bits().clone())
        print(f"\nOBS {c.name} {name} {_fmt(ratios)}")
    same = [bool(torch.equal(a, b)) for a, b in zip(res["resident"], res["streamed"])]
    print(f"OBS {c.name} bitwise equal to uniir_attention_rel_fwd / _rel_bwd: out={same[0]} lse={same[1]} dqkv={same[2]} drel={same[3]}")


def test_a_backward_without_enough_scratch_is_counted_and_inside_the_bound():
    """a fresh stream whose registered scratch holds one float less than batch * ceil(seq / 128) * nbuckets * heads: the backward keeps
    one float atomic per (item, key block, head, bucket), uniir_reduce_stats counts it and names the request; with exactly that much
    it does not lapse.  Both results are inside the bound, dqkv is the same bit for bit."""
    from uniir_amd import _lib as L, ops
    lib = _lib()
    c = Case("rel-long-300-noscratch", "attn_rlong_dkdv_kernel<0>", "rel", 3, 2, 300, nbuckets=32)
    items = R.build_items(c, DEV)
    run = RunRelLong(c, items)
    run.forward()
    out_in, lse_in = _round_ref(c, [it.fwd_ref()[0] for it in items])
    refs, _ = _bwd_refs(items, out_in, lse_in)
    need = c.batch * 3 * c.nbuckets * c.heads * 4
    s = torch.cuda.Stream()
    handle = C.c_void_p(s.cuda_stream)
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)
    dqkv = []
    try:
        for nbytes, lapses in ((need - 4, 1), (need, 0)):
            L.check(lib.uniir_reduce_scratch(C.c_void_p(buf.data_ptr()), nbytes, handle), "reduce_scratch")
            torch.cuda.synchronize()
            ops.reset_reduce_stats()
            with torch.cuda.stream(s):          # the buffers are filled on the stream the kernels run on
                run.backward(out_in, lse_in, stream=handle)
            assert ops.reduce_stats() == (lapses, need), (nbytes, ops.reduce_stats())
            ratios = {}
            _drel_judge(c, run, items, refs, ratios, f"scratch of {nbytes} bytes")
            dqkv.append(run.dX.bits().clone())
            print(f"\nOBS {c.name} scratch={nbytes} lapses={lapses} {_fmt(ratios)}")
        assert torch.equal(dqkv[0], dqkv[1])
    finally:
        torch.cuda.synchronize()
        L.check(lib.uniir_reduce_scratch(None, 0, handle), "reduce_scratch")
        ops.reset_reduce_stats()


def _reject_args():
    """(name, entry point, expected code, arguments without the stream); every pointer is a valid, aligned buffer unless the case is
    about it"""
    H, W = 2, 128
    big = torch.zeros(1100 * 3 * W + 64, dtype=BF, device=DEV)
    outb = torch.full((1100 * 3 * W + 64,), float("nan"), dtype=BF, device=DEV)
    lse = torch.full((4096,), float("nan"), dtype=torch.float32, device=DEV)
    ints = torch.ones(4200, dtype=torch.int32, device=DEV)
    emb = torch.zeros(128 * H, dtype=torch.float32, device=DEV)
    drel = torch.full((128 * H,), float("nan"), dtype=torch.float32, device=DEV)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)          # noqa: E731
    b, o, L, I, E, G = P(big), P(outb), P(lse), P(ints), P(emb), P(drel)

    def fw(seq=16, nb=32, p=0.0, batch=1, heads=H, qkv=b, out=o, lse_=L, emb_=E, tab=I):
        return [qkv, out, lse_, emb_, tab, nb, 1.0, batch, seq, heads, p, 1]

    def bw(seq=16, nb=32, p=0.0, batch=1, heads=H, qkv=b, out=b, dout=b, lse_=L, dqkv=o, emb_=E, tab=I):
        return [qkv, out, dout, lse_, dqkv, emb_, tab, nb, 1.0, G, batch, seq, heads, p, 1]

    F, B = "uniir_attention_rel_fwd_long", "uniir_attention_rel_bwd_long"
    t = [
        ("fwd-seq-0", F, "ESHAPE", fw(seq=0)), ("bwd-seq-0", B, "ESHAPE", bw(seq=0)),
        ("fwd-seq-1025", F, "ESHAPE", fw(seq=1025)), ("bwd-seq-1025", B, "ESHAPE", bw(seq=1025)),
        ("fwd-buckets-65", F, "EINVAL", fw(nb=65)), ("bwd-buckets-65", B, "EINVAL", bw(nb=65)),
        ("fwd-buckets-0", F, "EINVAL", fw(nb=0)), ("bwd-buckets-0", B, "EINVAL", bw(nb=0)),
        ("fwd-drop-1", F, "EINVAL", fw(p=1.0)), ("bwd-drop-1", B, "EINVAL", bw(p=1.0)),
        ("fwd-drop-neg", F, "EINVAL", fw(p=-0.1)), ("bwd-drop-neg", B, "EINVAL", bw(p=-0.1)),
        ("fwd-qkv-null", F, "EINVAL", fw(qkv=None)), ("bwd-qkv-null", B, "EINVAL", bw(qkv=None)),
        ("fwd-out-null", F, "EINVAL", fw(out=None)), ("bwd-dout-null", B, "EINVAL", bw(dout=None)),
        ("fwd-lse-null", F, "EINVAL", fw(lse_=None)), ("bwd-dqkv-null", B, "EINVAL", bw(dqkv=None)),
        ("fwd-emb-null", F, "EINVAL", fw(emb_=None)), ("bwd-bucket-null", B, "EINVAL", bw(tab=None)),
        ("fwd-heads-0", F, "EINVAL", fw(heads=0)), ("bwd-batch-neg", B, "EINVAL", bw(batch=-1)),
        ("fwd-qkv-misaligned", F, "EALIGN", fw(qkv=P(big, 8))), ("bwd-qkv-misaligned", B, "EALIGN", bw(qkv=P(big, 8))),
        ("fwd-out-misaligned", F, "EALIGN", fw(out=P(outb, 2))), ("bwd-dqkv-misaligned", B, "EALIGN", bw(dqkv=P(outb, 4))),
        ("bwd-dout-misaligned", B, "EALIGN", bw(dout=P(big, 8))),
        ("fwd-batch-0", F, "OK", fw(batch=0)), ("bwd-batch-0", B, "OK", bw(batch=0)),
    ]
    return t, (outb, lse, drel)


def test_rejections():
    """the documented code, and nothing written (batch == 0 is no error and writes nothing either)"""
    table, outs = _reject_args()
    lib = _lib()
    codes = dict(ERR, OK=0)
    wrong = []
    for name, fn, code, args in table:
        rc = getattr(lib, fn)(*args, _stream())
        torch.cuda.synchronize()
        if rc != codes[code]:
            wrong.append((name, fn, code, rc))
    assert not wrong, wrong
    assert all(bool(torch.isnan(t).all()) for t in outs), "a refused call wrote to an output"


def test_the_older_entry_points_still_stop_at_512():
    """the relative bias above 512 is the new entry points' alone: uniir_attention_rel_fwd / _rel_bwd refuse what they refused before"""
    H, W = 2, 128
    big = torch.zeros(520 * 3 * W, dtype=BF, device=DEV)
    outb = torch.full((520 * 3 * W,), float("nan"), dtype=BF, device=DEV)
    lse = torch.full((2048,), float("nan"), dtype=torch.float32, device=DEV)
    ints = torch.ones(1100, dtype=torch.int32, device=DEV)
    emb = torch.zeros(32 * H, dtype=torch.float32, device=DEV)
    drel = torch.full((32 * H,), float("nan"), dtype=torch.float32, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    lib = _lib()
    assert lib.uniir_attention_rel_fwd(P(big), P(outb), P(lse), P(emb), P(ints), 32, 1.0, 1, 513, H, 0.0, 1, _stream()) == ERR["ESHAPE"]
    assert lib.uniir_attention_rel_bwd(P(big), P(big), P(big), P(lse), P(outb), P(emb), P(ints), 32, 1.0, P(drel), 1, 513, H, 0.0, 1,
                                       _stream()) == ERR["ESHAPE"]
    torch.cuda.synchronize()
    assert bool(torch.isnan(outb).all()) and bool(torch.isnan(lse).all()) and bool(torch.isnan(drel).all())
