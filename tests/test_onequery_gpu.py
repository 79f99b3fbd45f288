"""uniir_onequery_fwd / _bwd -- ONE query row per item that stands for row drop_q of a call with drop_tq query rows: key counts, packed
keys and dropout in the one-query form (BLIP's last BERT layer on the class row) -- over the case table of tests/onequery_cases.py:
  forward and backward against the fp64 reference of tests/attention_ref.py, element by element inside the derived bounds, with the
  guarded buffers of tests/test_attention_paths_gpu.py: every element outside the logical extent -- pad columns, the other thirds of
  a [q | k | v] shaped buffer, the guard rows behind the last item -- must come back bit for bit; the backward runs on the rounded
  REFERENCE out / lse, twice, with equal bits; dense keys at or behind key_len get exact zeros in dk / dv;
  out and lse bit for bit row drop_q of the full call on the same operands and seed with tq = drop_tq: uniir_attention_fwd_ex (up to
  512 keys) or uniir_attention_fwd_long (above) with key_len -- for a packed case on the dense twin whose rows behind the item's length
  hold values that would take over the row -- and, for packed keys up to 512, row 0 of uniir_attention_fwd_rows with kv_packed = 1
  (tq = tk = drop_tq, the call BLIP's packed BERT makes);
  without key_len, packed keys and dropout both entry points equal uniir_attention_one_fwd / _one_bwd bit for bit.
One OBS line per case and direction holds the largest |got - ref| / bound of every output."""
import ctypes as C
import faulthandler

import pytest
import torch

import attention_ref as R
from onequery_cases import CASES, FULL_TQ, NAMES, PAD, build_items
from test_attention_paths_gpu import DEV, DROP_SEED, TAIL, Buf, _dropf, _fmt, _i32, _judge, _lib, _masked_keys_zero, _stream, _untouched

pytestmark = pytest.mark.gpu
CASE_SECONDS = 120
BF = torch.bfloat16


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _items(c):
    return build_items(c, DEV, _dropf(c.drop_p) if c.drop_p > 0 else None)


def P(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


class Fused(Buf):
    """a [rows][3 W] buffer whose logical extent is the K and V thirds of every row and, with `qrows`, the Q third of those rows"""

    def __init__(self, rows, W, qrows=()):
        super().__init__(rows, 3 * W, 3 * W, BF)
        self.W, self.qrows = W, list(qrows)

    def outside(self):
        m = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        m.as_strided((self.rows, 2 * self.W), (3 * self.W, 1), self.W).fill_(False)
        for r in self.qrows:
            m[r * 3 * self.W:r * 3 * self.W + self.W] = False
        return m


class RunQ:
    """the buffers of one case in its layout (onequery_cases) and the two calls"""

    def __init__(self, c, items):
        self.c, self.items = c, items
        self.W = W = c.heads * 64
        self.fused = c.layout == "qkv"
        self.klen = [it.Tk for it in items]                       # rows of k / v the item owns
        self.k0 = [sum(self.klen[:m]) for m in range(c.batch + 1)]
        nk = self.k0[-1]
        self.key_len = _i32(c.lens) if c.form == "klen" else None
        self.kv_row_off = _i32(self.k0) if c.form == "packed" else None
        self.q_in_x = self.fused and c.form != "packed"           # q = row m * tk of the [q | k | v] buffer
        if self.fused:
            self.KV, self.kcol, self.kv_ld, self.dkv_ld = Fused(nk, W, [m * c.tk for m in range(c.batch)] if self.q_in_x else ()), W, 3 * W, 3 * W
            self.out_ld = W
        else:
            self.KV, self.kcol, self.kv_ld, self.dkv_ld = Buf(nk, 2 * W, 2 * W + PAD, BF), 0, 2 * W + PAD, 2 * W + PAD + 24
            self.out_ld = W + PAD + 8
        if self.q_in_x:
            self.Q, self.q_ld, self.dq_ld = None, c.tk * 3 * W, c.tk * 3 * W
        else:
            self.q_ld = W if self.fused else W + PAD
            self.Q, self.dq_ld = Buf(c.batch, W, self.q_ld, BF), W + PAD + 16
        for m, it in enumerate(items):
            rows = self.KV.view[self.k0[m]:self.k0[m + 1]]
            rows[:, self.kcol:self.kcol + W], rows[:, self.kcol + W:self.kcol + 2 * W] = it.k.reshape(-1, W), it.v.reshape(-1, W)
            if self.q_in_x:
                self.KV.view[m * c.tk, :W] = it.q.reshape(W)
            else:
                self.Q.view[m] = it.q.reshape(W)

    def _q(self):
        return self.KV.ptr(0) if self.q_in_x else self.Q.ptr()

    def _tail(self):
        c = self.c
        kl = None if self.key_len is None else P(self.key_len)
        ro = None if self.kv_row_off is None else P(self.kv_row_off)
        return kl, ro

    def forward(self):
        c, W = self.c, self.W
        self.out = Buf(c.batch, W, self.out_ld, BF)
        self.lse = Buf(1, c.batch * c.heads, c.batch * c.heads + TAIL, torch.float32)
        before = {"out": self.out.bits().clone(), "lse": self.lse.bits().clone()}
        kl, ro = self._tail()
        rc = _lib().uniir_onequery_fwd(self._q(), self.q_ld, self.KV.ptr(self.kcol), self.KV.ptr(self.kcol + W), self.kv_ld, self.out.ptr(),
                                       self.out_ld, self.lse.ptr(), kl, ro, c.batch, c.tk, c.heads, c.drop_p, DROP_SEED, c.drop_tq,
                                       c.drop_q, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        _untouched(f"{c.name} out", self.out, before["out"])
        _untouched(f"{c.name} lse", self.lse, before["lse"])
        lse = self.lse.view[0].view(c.batch, c.heads)
        return [{"out": self.out.view[m].reshape(1, c.heads, 64), "lse": lse[m].reshape(c.heads, 1)} for m in range(c.batch)]

    def backward(self, out_in, lse_in):
        c, W = self.c, self.W
        O, dO = Buf(c.batch, W, self.out_ld, BF), Buf(c.batch, W, self.out_ld, BF)
        L = Buf(1, c.batch * c.heads, c.batch * c.heads + TAIL, torch.float32)
        for m, it in enumerate(self.items):
            O.view[m], dO.view[m] = out_in[m].reshape(W), it.dout.reshape(W)
            L.view[0].view(c.batch, c.heads)[m] = lse_in[m].reshape(c.heads)
        nk = self.k0[-1]
        if self.fused:
            self.dKV = Fused(nk, W, [m * c.tk for m in range(c.batch)] if self.q_in_x else ())
        else:
            self.dKV = Buf(nk, 2 * W, self.dkv_ld, BF)
        self.dQ = None if self.q_in_x else Buf(c.batch, W, self.dq_ld, BF)
        outs = {"dkv": self.dKV} if self.q_in_x else {"dq": self.dQ, "dkv": self.dKV}
        before = {k: b.bits().clone() for k, b in outs.items()}
        kl, ro = self._tail()
        dq = self.dKV.ptr(0) if self.q_in_x else self.dQ.ptr()
        rc = _lib().uniir_onequery_bwd(self._q(), self.q_ld, self.KV.ptr(self.kcol), self.KV.ptr(self.kcol + W), self.kv_ld, O.ptr(), dO.ptr(),
                                       self.out_ld, L.ptr(), kl, ro, dq, self.dq_ld, self.dKV.ptr(self.kcol), self.dKV.ptr(self.kcol + W),
                                       self.dkv_ld, c.batch, c.tk, c.heads, c.drop_p, DROP_SEED, c.drop_tq, c.drop_q, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        for name, b in outs.items():
            _untouched(f"{c.name} {name}", b, before[name])
        res = []
        for m in range(c.batch):
            kv = self.dKV.view[self.k0[m]:self.k0[m + 1]]
            dqm = self.dKV.view[m * c.tk:m * c.tk + 1, :W] if self.q_in_x else self.dQ.view[m:m + 1]
            d = {"dq": dqm, "dk": kv[:, self.kcol:self.kcol + W], "dv": kv[:, self.kcol + W:self.kcol + 2 * W]}
            res.append({k: t.reshape(t.shape[0], c.heads, 64) for k, t in d.items()})
        return res

    def grad_bits(self):
        return [b.bits().clone() for b in (self.dQ, self.dKV) if b is not None]


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_onequery_path(case):
    c = case
    items = _items(c)
    run = RunQ(c, items)
    ratios = {}
    fref = [it.fwd_ref()[0] for it in items]
    _judge(c, "forward", run.forward(), fref, ratios)
    print(f"\nOBS {c.name} [{c.path}] forward {_fmt(ratios)}")
    out_in, lse_in = [f["out"][0].to(BF) for f in fref], [f["lse"][0].float() for f in fref]
    dref = [{k: v for k, v in it.bwd_ref(o, l).items() if k in ("dq", "dk", "dv")} for it, o, l in zip(items, out_in, lse_in)]
    ratios = {}
    got = run.backward(out_in, lse_in)
    _judge(c, "backward", got, dref, ratios)
    _masked_keys_zero(c, items, got)
    print(f"OBS {c.name} [{c.path}] backward {_fmt(ratios)}")
    bits = run.grad_bits()
    run.backward(out_in, lse_in)
    assert all(torch.equal(a, b) for a, b in zip(run.grad_bits(), bits)), f"{c.name}: the backward differs between two runs"


def _one_call(c, q, k, v, kv_ld, *, key_len=None, kv_row_off=None, drop_tq=None, drop_q=None):
    """uniir_onequery_fwd on plain tensors: q [batch][W] -> out [batch][W], lse [batch][H]"""
    W = c.heads * 64
    out = torch.empty(c.batch, W, device=DEV, dtype=BF)
    lse = torch.empty(c.batch, c.heads, device=DEV, dtype=torch.float32)
    rc = _lib().uniir_onequery_fwd(P(q), W, k, v, kv_ld, P(out), W, P(lse), None if key_len is None else P(key_len),
                                   None if kv_row_off is None else P(kv_row_off), c.batch, c.tk, c.heads, c.drop_p, DROP_SEED,
                                   c.drop_tq if drop_tq is None else drop_tq, c.drop_q if drop_q is None else drop_q, _stream())
    torch.cuda.synchronize()
    assert rc == 0, (c.name, rc)
    return out, lse


def _same(c, what, out1, lse1, out_full, lse_full):
    assert torch.equal(out1.view(torch.int16), out_full.contiguous().view(torch.int16)), f"{c.name}: out differs from {what}"
    assert torch.equal(lse1.view(torch.int32), lse_full.contiguous().view(torch.int32)), f"{c.name}: lse differs from {what}"


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_forward_is_row_drop_q_of_the_full_call(case):
    c = case
    items = _items(c)
    W, T, lib = c.heads * 64, c.tk, _lib()
    tq = c.drop_tq
    # the full call's operands: dense [batch][tq] queries (row drop_q of every item is the query), dense [batch][tk] keys (the twin's)
    qf = torch.empty(c.batch, tq, W, device=DEV, dtype=BF)
    kvf = torch.empty(c.batch * T, 2 * W, device=DEV, dtype=BF)
    for m, it in enumerate(items):
        qf[m] = it.twin[0].reshape(FULL_TQ, W) if tq == FULL_TQ else it.q.reshape(1, W)
        kvf[m * T:(m + 1) * T, :W], kvf[m * T:(m + 1) * T, W:] = it.twin[1].reshape(T, W), it.twin[2].reshape(T, W)
    assert all(torch.equal(qf[m, c.drop_q], it.q.reshape(W)) for m, it in enumerate(items))
    key_len = None if c.lens is None else _i32(c.lens)
    out = torch.empty(c.batch * tq, W, device=DEV, dtype=BF)
    lse = torch.empty(c.batch, c.heads, tq, device=DEV, dtype=torch.float32)
    kl = None if key_len is None else P(key_len)
    if T <= 512:
        rc = lib.uniir_attention_fwd_ex(P(qf), W, P(kvf), P(kvf, W * 2), 2 * W, P(out), W, P(lse), kl, c.batch, tq, T, c.heads, 0, c.drop_p,
                                        DROP_SEED, _stream())
    else:
        rc = lib.uniir_attention_fwd_long(P(qf), W, P(kvf), P(kvf, W * 2), 2 * W, P(out), W, P(lse), None, kl, c.batch, tq, T, c.heads,
                                          c.drop_p, DROP_SEED, _stream())
    assert rc == 0, rc
    q1 = qf[:, c.drop_q].contiguous()
    if c.form == "packed":
        lens = [it.Tk for it in items]
        off = [sum(lens[:m]) for m in range(c.batch + 1)]
        kvp = torch.cat([kvf[m * T:m * T + lens[m]] for m in range(c.batch)]).contiguous()
        row_off = _i32(off)
        out1, lse1 = _one_call(c, q1, P(kvp), P(kvp, W * 2), 2 * W, kv_row_off=row_off)
    else:
        out1, lse1 = _one_call(c, q1, P(kvf), P(kvf, W * 2), 2 * W, key_len=key_len)
    _same(c, "the dense full call", out1, lse1, out.view(c.batch, tq, W)[:, c.drop_q], lse[:, :, c.drop_q])
    if c.form == "packed" and T <= 512:
        # the packed BERT's own call: packed [q | k | v] rows, tq = tk = the dropout stride, the class row is row 0 of every item
        X = torch.randn(off[-1], 3 * W, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3)).to(BF)
        X[:, W:] = kvp
        for m in range(c.batch):
            X[off[m], :W] = q1[m]
        outp = torch.empty(off[-1], W, device=DEV, dtype=BF)
        lsep = torch.empty(c.batch, c.heads, T, device=DEV, dtype=torch.float32)
        rc = lib.uniir_attention_fwd_rows(P(X), 3 * W, P(X, W * 2), P(X, W * 4), 3 * W, P(outp), W, P(lsep), P(row_off), 1, None, c.batch, T, T,
                                          c.heads, c.drop_p, DROP_SEED, _stream())
        assert rc == 0, rc
        out1, lse1 = _one_call(c, q1, P(X, W * 2), P(X, W * 4), 3 * W, kv_row_off=row_off, drop_tq=T, drop_q=0)
        _same(c, "uniir_attention_fwd_rows (kv_packed)", out1, lse1, outp[torch.tensor(off[:-1], device=DEV)], lsep[:, :, 0])


PLAIN = [c for c in CASES if c.form == "dense" and c.drop_p == 0]


@pytest.mark.parametrize("case", PLAIN, ids=[c.name for c in PLAIN])
def test_without_mask_and_dropout_it_is_uniir_attention_one(case):
    c = case
    items = _items(c)
    W, T, lib = c.heads * 64, c.tk, _lib()
    q = torch.stack([it.q.reshape(W) for it in items]).contiguous()
    kv = torch.cat([torch.cat([it.k.reshape(T, W), it.v.reshape(T, W)], 1) for it in items]).contiguous()
    fref = [it.fwd_ref()[0] for it in items]
    o_in = torch.stack([f["out"][0].to(BF).reshape(W) for f in fref]).contiguous()
    l_in = torch.stack([f["lse"][0].float().reshape(c.heads) for f in fref]).contiguous()
    do = torch.stack([it.dout.reshape(W) for it in items]).contiguous()
    res = []
    for new in (False, True):
        out = torch.empty(c.batch, W, device=DEV, dtype=BF)
        lse = torch.empty(c.batch, c.heads, device=DEV, dtype=torch.float32)
        dq = torch.zeros(c.batch, W, device=DEV, dtype=BF)
        dkv = torch.zeros(c.batch * T, 2 * W, device=DEV, dtype=BF)
        if new:
            rc = lib.uniir_onequery_fwd(P(q), W, P(kv), P(kv, W * 2), 2 * W, P(out), W, P(lse), None, None, c.batch, T, c.heads, 0.0, 0,
                                        c.drop_tq, c.drop_q, _stream())
            assert rc == 0, rc
            rc = lib.uniir_onequery_bwd(P(q), W, P(kv), P(kv, W * 2), 2 * W, P(o_in), P(do), W, P(l_in), None, None, P(dq), W, P(dkv),
                                        P(dkv, W * 2), 2 * W, c.batch, T, c.heads, 0.0, 0, c.drop_tq, c.drop_q, _stream())
        else:
            rc = lib.uniir_attention_one_fwd(P(q), P(kv), P(kv, W * 2), 2 * W, P(out), P(lse), c.batch, T, c.heads, 0, _stream())
            assert rc == 0, rc
            rc = lib.uniir_attention_one_bwd(P(q), P(kv), P(kv, W * 2), 2 * W, P(o_in), P(do), P(l_in), P(dq), W, P(dkv), P(dkv, W * 2), 2 * W,
                                             c.batch, T, c.heads, _stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        res.append((out.view(torch.int16), lse.view(torch.int32), dq.view(torch.int16), dkv.view(torch.int16)))
    for name, a, b in zip(("out", "lse", "dq", "dk | dv"), *res):
        assert torch.equal(a, b), f"{c.name}: {name} differs from uniir_attention_one_fwd / _one_bwd"
