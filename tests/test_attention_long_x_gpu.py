"""uniir_attention_fwd_long / _bwd_long -- the general attention form (Q separate from K | V, key_len, dropout, packed query rows) for
1 <= tq, tk <= 1024 on the streaming kernels attn_xlong_* of csrc/attention_long.hip -- against the fp64 reference of
tests/attention_ref.py, element by element, with the machinery and the requirements of tests/test_attention_paths_gpu.py:
  every output of every item inside its bound; every tensor has a NaN guard band, every leading dimension is wider than the row
  (pad = 72), and everything outside the logical extent -- the lse entries of the rows a packed item does not have included -- comes
  back bit for bit; forward and backward run twice and are compared with torch.equal; the backward runs on the rounded REFERENCE
  out / lse and, for `chained` cases, once more on the kernel's own forward; dk / dv of masked keys are exactly zero; the live rows
  of a packed call equal, bit for bit, the same entry point called dense (q_row_off = NULL) on the padded twin with zero dout on the
  padding rows and the case's own key_len.  One OBS line per case holds the largest |got - ref| / bound of every output.
The case table (tests/attention_long_x_cases.py) is checked on the CPU by tests/test_attention_long_x_ref.py.
Further: the plain square call on a packed qkv buffer against uniir_attention_fwd / _bwd (same bounds; whether the bits agree is
printed, not asserted), and the calls the entry points refuse on the host."""
import ctypes as C
import faulthandler

import pytest
import torch

import attention_ref as R
from attention_long_x_cases import CASES, NAMES
from attention_ref import Case
from test_attention_paths_gpu import (DEV, DROP_SEED, ERR, TAIL, Buf, Run, _bwd_refs, _dropf, _fmt, _i32, _judge, _lib,
                                      _masked_keys_zero, _round_ref, _stream, _untouched)

pytestmark = pytest.mark.gpu
CASE_SECONDS = 120    # a case takes a few seconds; a hung kernel ends the run here instead of at the runner's limit
BF = torch.bfloat16


class RunLong(Run):
    """the buffers of Run, the calls of the new entry points.  dense: the padded twin of a packed case -- q_row_off = NULL, key_len as
    the case gives it.  A case of api "qkv" keeps Run's packed qkv buffer: q | k | v are views of it."""

    def __init__(self, c, items, dense=False):
        super().__init__(c, items, dense)
        self.key_len = None if c.key_len is None else _i32(c.key_len)

    def _opt(self):
        kl = None if self.key_len is None else C.c_void_p(self.key_len.data_ptr())
        ro = None if self.row_off is None else C.c_void_p(self.row_off.data_ptr())
        return ro, kl

    def forward(self):
        c, lib, W = self.c, _lib(), self.W
        self.out = Buf(self.nq, W, self.out_ld, c.dtype)
        self.lse = Buf(1, c.batch * c.heads * c.tq, c.batch * c.heads * c.tq + TAIL, torch.float32)
        before = {"out": self.out.bits().clone(), "lse": self.lse.bits().clone()}
        q, k, v = self._qkv()
        ro, kl = self._opt()
        rc = lib.uniir_attention_fwd_long(q, self.q_ld, k, v, self.kv_ld, self.out.ptr(), self.out_ld, self.lse.ptr(), ro, kl, c.batch,
                                          c.tq, c.tk, c.heads, c.drop_p, DROP_SEED, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        _untouched(f"{c.name} out", self.out, before["out"])
        dead = torch.ones(self.lse.flat.numel(), dtype=torch.bool, device=DEV)
        dead[:c.batch * c.heads * c.tq] = ~self.live_lse().flatten()
        _untouched(f"{c.name} lse", self.lse, before["lse"], dead & ~self.lse.outside())
        return self.item_outputs_fwd()

    def backward(self, out_in, lse_in, dout=None):
        c, lib, W = self.c, _lib(), self.W
        O, dO = Buf(self.nq, W, self.out_ld, c.dtype), Buf(self.nq, W, self.out_ld, c.dtype)
        L = Buf(1, c.batch * c.heads * c.tq, c.batch * c.heads * c.tq + TAIL, torch.float32)
        lview = L.view[0].view(c.batch, c.heads, c.tq)
        for m, it in enumerate(self.items):
            lq = self.qlen[m]
            O.view[self.q0[m]:self.q0[m] + lq] = out_in[m].reshape(lq, W)
            dO.view[self.q0[m]:self.q0[m] + lq] = (it.twin[3][:lq] if dout is None else dout[m]).reshape(lq, W)
            lview[m, :, :lq] = lse_in[m]
        if self.fused:
            self.dX = Buf(self.nq, 3 * W, 3 * W, c.dtype)
            dq, dk, dv = self.dX.ptr(0), self.dX.ptr(W), self.dX.ptr(2 * W)
            outs = {"dqkv": self.dX}
        else:
            self.dQ, self.dKV = Buf(self.nq, W, self.dq_ld, c.dtype), Buf(self.nk, 2 * W, self.dkv_ld, c.dtype)
            dq, dk, dv = self.dQ.ptr(0), self.dKV.ptr(0), self.dKV.ptr(W)
            outs = {"dq": self.dQ, "dkv": self.dKV}
        before = {k: b.bits().clone() for k, b in outs.items()}
        q, k, v = self._qkv()
        ro, kl = self._opt()
        rc = lib.uniir_attention_bwd_long(q, self.q_ld, k, v, self.kv_ld, O.ptr(), dO.ptr(), self.out_ld, L.ptr(), ro, kl, dq, self.dq_ld,
                                          dk, dv, self.dkv_ld, c.batch, c.tq, c.tk, c.heads, c.drop_p, DROP_SEED, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        for name, b in outs.items():
            _untouched(f"{c.name} {name}", b, before[name])
        return self.item_outputs_bwd()

    def grad_bufs(self):
        return (self.dX,) if self.fused else (self.dQ, self.dKV)


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _forward_twice(c, run, items, ratios):
    got_f = run.forward()
    fref = [it.fwd_ref()[0] for it in items]
    _judge(c, "forward", got_f, fref, ratios)
    out_bits, lse_bits = run.out.bits().clone(), run.lse.bits().clone()
    own = [{k: v.clone() for k, v in g.items()} for g in got_f]
    run.forward()
    assert torch.equal(run.out.bits(), out_bits) and torch.equal(run.lse.bits(), lse_bits), f"{c.name}: the forward differs between two runs"
    return own, fref


def _backward_twice(c, run, items, what, o_in, l_in, ratios):
    got_b = run.backward(o_in, l_in)
    _, dref = _bwd_refs(items, o_in, l_in)
    _judge(c, what, got_b, dref, ratios)
    _masked_keys_zero(c, items, got_b)
    keep = [{k: v.clone() for k, v in g.items()} for g in got_b]
    bits = [b.bits().clone() for b in run.grad_bufs()]
    run.backward(o_in, l_in)
    for b, old in zip(run.grad_bufs(), bits):
        assert torch.equal(b.bits(), old), f"{c.name}: the {what} differs between two runs"
    return keep


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_attention_long_path(case):
    c = case
    items = R.build_items(c, DEV, _dropf(c.drop_p) if c.drop_p > 0 else None)
    run = RunLong(c, items)
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
    if c.lens is not None:
        _same_as_dense(c, items, run, own)


def _same_as_dense(c, items, run, own_f):
    """_same_as_dense of tests/test_attention_paths_gpu.py with the dense call made through the same entry point"""
    dense = RunLong(c, items, dense=True)
    assert dense.row_off is None and run.row_off is not None
    got_f = dense.forward()
    for m, it in enumerate(items):
        for name in ("out", "lse"):
            d = got_f[m][name][:it.Tq] if name == "out" else got_f[m][name][:, :it.Tq]
            assert torch.equal(d, own_f[m][name]), f"{c.name} item {m}: {name} of the packed call differs from the dense call"
    got_p = run.backward([g["out"] for g in own_f], [g["lse"] for g in own_f])
    got_p = [{k: v.clone() for k, v in g.items()} for g in got_p]
    got_d = dense.backward([g["out"] for g in got_f], [g["lse"] for g in got_f], dout=[it.twin[3] for it in items])
    for m, it in enumerate(items):
        for name, n in (("dq", it.Tq), ("dk", it.Tk), ("dv", it.Tk)):
            assert torch.equal(got_d[m][name][:n], got_p[m][name]), f"{c.name} item {m}: {name} of the packed call differs from the dense call"


def test_plain_square_call_fits_the_bounds_of_the_self_attention_entry_points():
    """2 items, 2 heads, 577 x 577, no key_len, no q_row_off, no dropout, q | k | v views of one packed qkv buffer: the new forward and
    backward fit the bounds uniir_attention_fwd / _bwd are held to on that buffer.  Whether the bits agree is an observation."""
    c = Case("plain-577", "attn_long_* | attn_xlong_*<0>", "qkv", 2, 2, 577)
    items = R.build_items(c, DEV)
    old, new = Run(c, items), RunLong(c, items)
    assert new.fused and new.q_ld == new.kv_ld == 3 * new.W and new.out_ld == new.W
    res = {}
    for name, run in (("self", old), ("long", new)):
        ratios = {}
        got_f = run.forward()
        fref = [it.fwd_ref()[0] for it in items]
        _judge(c, f"{name} forward", got_f, fref, ratios)
        out_in, lse_in = _round_ref(c, fref)
        got_b = run.backward(out_in, lse_in)
        _, dref = _bwd_refs(items, out_in, lse_in)
        _judge(c, f"{name} backward", got_b, dref, ratios)
        res[name] = (run.out.bits().clone(), run.lse.bits().clone(), run.dX.bits().clone())
        print(f"\nOBS plain-577 {name} {_fmt(ratios)}")
    same = [bool(torch.equal(a, b)) for a, b in zip(res["self"], res["long"])]
    print(f"OBS plain-577 bitwise equal to uniir_attention_fwd / _bwd: out={same[0]} lse={same[1]} dqkv={same[2]}")


def _reject_args():
    """(name, entry point, expected code, arguments without the stream); every pointer is a valid, aligned buffer unless the case is
    about it"""
    H, W = 2, 128
    big = torch.zeros(1100 * 3 * W + 64, dtype=BF, device=DEV)
    outb = torch.full((1100 * 3 * W + 64,), float("nan"), dtype=BF, device=DEV)
    lse = torch.full((4096,), float("nan"), dtype=torch.float32, device=DEV)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)          # noqa: E731
    b, o, L = P(big), P(outb), P(lse)

    def fw(tq=16, tk=16, q_ld=W, kv_ld=2 * W, out_ld=W, q=b, p=0.0, batch=1):
        return [q, q_ld, b, b, kv_ld, o, out_ld, L, None, None, batch, tq, tk, H, p, 1]

    def bw(tq=16, tk=16, q_ld=W, kv_ld=2 * W, out_ld=W, dq_ld=W, dkv_ld=2 * W, q=b, dq=o, p=0.0, batch=1):
        return [q, q_ld, b, b, kv_ld, b, b, out_ld, L, None, None, dq, dq_ld, o, o, dkv_ld, batch, tq, tk, H, p, 1]

    F, B = "uniir_attention_fwd_long", "uniir_attention_bwd_long"
    t = [
        ("fwd-tq-1025", F, "ESHAPE", fw(tq=1025)), ("bwd-tq-1025", B, "ESHAPE", bw(tq=1025)),
        ("fwd-tk-1025", F, "ESHAPE", fw(tk=1025)), ("bwd-tk-1025", B, "ESHAPE", bw(tk=1025)),
        ("fwd-tq-0", F, "ESHAPE", fw(tq=0)), ("bwd-tq-0", B, "ESHAPE", bw(tq=0)),
        ("fwd-q_ld-132", F, "EALIGN", fw(q_ld=W + 4)), ("bwd-q_ld-132", B, "EALIGN", bw(q_ld=W + 4)),
        ("fwd-kv_ld-260", F, "EALIGN", fw(kv_ld=2 * W + 4)), ("bwd-kv_ld-260", B, "EALIGN", bw(kv_ld=2 * W + 4)),
        ("fwd-out_ld-129", F, "EALIGN", fw(out_ld=W + 1)), ("bwd-out_ld-129", B, "EALIGN", bw(out_ld=W + 1)),
        ("bwd-dq_ld-132", B, "EALIGN", bw(dq_ld=W + 4)),
        ("bwd-dkv_ld-258", B, "EALIGN", bw(dkv_ld=2 * W + 2)),
        ("fwd-q-misaligned", F, "EALIGN", fw(q=P(big, 8))), ("bwd-q-misaligned", B, "EALIGN", bw(q=P(big, 8))),
        ("bwd-dq-misaligned", B, "EALIGN", bw(dq=P(outb, 2))),
        ("fwd-q-null", F, "EINVAL", fw(q=None)), ("bwd-q-null", B, "EINVAL", bw(q=None)),
        ("fwd-drop-1", F, "EINVAL", fw(p=1.0)), ("bwd-drop-1", B, "EINVAL", bw(p=1.0)),
        ("fwd-drop-neg", F, "EINVAL", fw(p=-0.1)), ("bwd-drop-neg", B, "EINVAL", bw(p=-0.1)),
        ("fwd-batch-neg", F, "EINVAL", fw(batch=-1)),
        ("fwd-batch-0", F, "OK", fw(batch=0)), ("bwd-batch-0", B, "OK", bw(batch=0)),
    ]
    return t, (outb, lse)


def test_rejections():
    """the documented code, and nothing written (batch == 0 is no error and writes nothing either)"""
    table, (outb, lse) = _reject_args()
    lib = _lib()
    codes = dict(ERR, OK=0)
    wrong = []
    for name, fn, code, args in table:
        rc = getattr(lib, fn)(*args, _stream())
        torch.cuda.synchronize()
        if rc != codes[code]:
            wrong.append((name, fn, code, rc))
    assert not wrong, wrong
    assert bool(torch.isnan(outb).all()) and bool(torch.isnan(lse).all()), "a refused call wrote to an output"


def test_the_older_entry_points_still_stop_at_512():
    """the general form above 512 is the new entry points' alone: _ex / _rows refuse what they refused before"""
    H, W = 2, 128
    big = torch.zeros(600 * 3 * W, dtype=BF, device=DEV)
    outb = torch.full((600 * W,), float("nan"), dtype=BF, device=DEV)
    lse = torch.full((2048,), float("nan"), dtype=torch.float32, device=DEV)
    ro = _i32([0, 16])
    P = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    lib = _lib()
    assert lib.uniir_attention_fwd_ex(P(big), W, P(big), P(big), 2 * W, P(outb), W, P(lse), None, 1, 16, 513, H, 0, 0.0, 1, _stream()) == ERR["ESHAPE"]
    assert lib.uniir_attention_fwd_rows(P(big), W, P(big), P(big), 2 * W, P(outb), W, P(lse), P(ro), 0, None, 1, 16, 513, H, 0.0, 1,
                                        _stream()) == ERR["ESHAPE"]
    torch.cuda.synchronize()
    assert bool(torch.isnan(outb).all()) and bool(torch.isnan(lse).all())
