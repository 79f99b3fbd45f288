"""uniir_attn_general_fwd_f16 and uniir_onequery_fwd_f16 on the device: every case of tests/attn_general_f16_cases.py element by
element against the fp64 reference and the derived bound of tests/attention_ref.py with torch.float16 (fp16's unit roundoff and the
ETA_P term for the unnormalised P).  No element is excluded from a comparison.

Calls go through the ctypes handle with the test's own buffers, as in tests/test_attention_paths_gpu.py: every tensor has a guard
band behind it, every leading dimension is wider than the row, and everything outside the logical extent -- the lse entries of rows
a packed item does not have included -- holds a NaN pattern that must come back bit for bit.  Beyond the bound:
  two calls on the same operands give the same bits;
  a packed call's live rows are torch.equal to the dense padded call's rows;
  the one-query form is torch.equal to row 0 of the full call on the same operands;
  up to 512, with tq == tk, no key_len and the Q / K / V thirds of one packed buffer, the call is torch.equal to
  uniir_attention_fwd_f16 (the same kernel); above 512 the two are different kernels, both inside the bound, and the test prints
  whether their bits agree.
Each case prints an OBS line with the largest |got - ref| / bound of its outputs."""
import ctypes as C
import faulthandler

import pytest
import torch

import attention_ref as R
from attention_ref import Case
from attn_general_f16_cases import CASES, NAMES, ONEQ, ONEQ_NAMES, PAD, oneq_full_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16 = torch.float16
GUARD = 24            # rows of guard band behind every tensor
TAIL = 64             # spare floats behind lse
NAN16, NAN32 = 0x7E01, 0x7FC00011
CASE_SECONDS = 120    # a case takes a few seconds; a hung kernel ends the run here instead of at the runner's limit


def _lib():
    from uniir_amd import _lib
    return _lib.load()


def _stream():
    from uniir_amd import ops
    return ops._stream()


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


class Buf:
    """a [rows][cols] view of pitch ld with GUARD rows behind it; every element outside the view holds the NaN pattern"""

    def __init__(self, rows, cols, ld, dtype):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.ibits = {2: torch.int16, 4: torch.int32}[dtype.itemsize]
        self.flat = torch.empty((rows + GUARD) * ld, dtype=dtype, device=DEV)
        self.flat.view(self.ibits).fill_(NAN16 if dtype.itemsize == 2 else NAN32)
        self.view = self.flat.as_strided((rows, cols), (ld, 1))

    def ptr(self, col=0, row=0):
        return C.c_void_p(self.flat.data_ptr() + (row * self.ld + col) * self.dtype.itemsize)

    def bits(self):
        return self.flat.view(self.ibits)

    def outside(self):
        m = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        m.as_strided((self.rows, self.cols), (self.ld, 1)).fill_(False)
        return m


def _untouched(name, buf, before, extra_mask=None):
    mask = buf.outside()
    if extra_mask is not None:
        mask = mask | extra_mask
    now = buf.bits()
    if not torch.equal(now[mask], before[mask]):
        raise AssertionError(f"{name}: {int((now[mask] != before[mask]).sum())} elements changed outside the logical extent")


def _i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device=DEV)


def _vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Run:
    """the buffers of one case and its call.  dense: the padded twin of a packed case (no q_row_off, the items' full tq / tk rows,
    key_len = the lengths the packed call implies)"""

    def __init__(self, c, items, dense=False):
        self.c, self.items, self.dense = c, items, dense
        self.W = W = c.heads * 64
        packed_q = c.lens is not None and not dense
        packed_k = packed_q and bool(c.kv_packed)
        self.qlen = [it.Tq if packed_q else c.tq for it in items]
        self.klen = [it.Tk if packed_k else c.tk for it in items]
        self.q0 = [sum(self.qlen[:m]) for m in range(c.batch + 1)]
        self.k0 = [sum(self.klen[:m]) for m in range(c.batch + 1)]
        self.row_off = _i32(self.q0) if packed_q else None
        self.kv_packed = int(packed_k)
        if dense:
            self.key_len = _i32([it.twin_key_len for it in items])
        else:
            self.key_len = None if c.key_len is None else _i32(c.key_len)
        self.nq, self.nk = self.q0[-1], self.k0[-1]
        self.q_ld, self.kv_ld, self.out_ld = W + PAD, 2 * W + PAD, W + PAD + 8
        self.Q = Buf(self.nq, W, self.q_ld, F16)
        self.KV = Buf(self.nk, 2 * W, self.kv_ld, F16)
        for m, it in enumerate(items):
            q, k, v, _ = it.twin
            lq, lk = self.qlen[m], self.klen[m]
            self.Q.view[self.q0[m]:self.q0[m] + lq] = q[:lq].reshape(lq, W)
            rows = self.KV.view[self.k0[m]:self.k0[m] + lk]
            rows[:, :W], rows[:, W:] = k[:lk].reshape(lk, W), v[:lk].reshape(lk, W)

    def live_lse(self):
        c = self.c
        m = torch.zeros(c.batch, c.heads, c.tq, dtype=torch.bool, device=DEV)
        for i, l in enumerate(self.qlen):
            m[i, :, :l] = True
        return m

    def forward(self):
        c, W = self.c, self.W
        self.out = Buf(self.nq, W, self.out_ld, F16)
        self.lse = Buf(1, c.batch * c.heads * c.tq, c.batch * c.heads * c.tq + TAIL, torch.float32)
        before = {"out": self.out.bits().clone(), "lse": self.lse.bits().clone()}
        rc = _lib().uniir_attn_general_fwd_f16(self.Q.ptr(), self.q_ld, self.KV.ptr(0), self.KV.ptr(W), self.kv_ld, self.out.ptr(),
                                               self.out_ld, self.lse.ptr(), _vp(self.row_off), self.kv_packed, _vp(self.key_len),
                                               c.batch, c.tq, c.tk, c.heads, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        _untouched(f"{c.name} out", self.out, before["out"])
        dead = torch.ones(self.lse.flat.numel(), dtype=torch.bool, device=DEV)
        dead[:c.batch * c.heads * c.tq] = ~self.live_lse().flatten()
        _untouched(f"{c.name} lse", self.lse, before["lse"], dead & ~self.lse.outside())
        lse = self.lse.view[0].view(c.batch, c.heads, c.tq)
        return [{"out": self.out.view[self.q0[m]:self.q0[m] + self.qlen[m]].reshape(self.qlen[m], c.heads, 64),
                 "lse": lse[m, :, :self.qlen[m]]} for m in range(c.batch)]


def _judge(c, what, got_items, ref_items, ratios):
    """every output of every item inside its bound, no element left out; ratios[name] collects the largest |got - ref| / bound"""
    for m, (got, ref) in enumerate(zip(got_items, ref_items)):
        for name, g in got.items():
            r, b = ref[name]
            assert g.numel() == r.numel()
            why = R.compare(g, r, b, torch.float32 if name == "lse" else F16)
            ratios[name] = max(ratios.get(name, 0.0), R.worst(g, r, b))
            assert why is None, f"{c.name} ({c.path}) {what} item {m} {name}: {why}"


def _fmt(ratios):
    return " ".join(f"{k}={v:.3f}" for k, v in ratios.items())


def _run_case(c):
    """-> (items, run, the call's outputs as clones, the references); judged, repeated, and compared with the dense twin when packed"""
    items = R.build_items(c, DEV)
    run = Run(c, items)
    got = run.forward()
    fref = [it.fwd_ref()[0] for it in items]
    ratios = {}
    _judge(c, "forward", got, fref, ratios)
    out_bits, lse_bits = run.out.bits().clone(), run.lse.bits().clone()
    run.forward()
    assert torch.equal(run.out.bits(), out_bits) and torch.equal(run.lse.bits(), lse_bits), f"{c.name}: two calls differ"
    print(f"\nOBS {c.name} [{c.path}] forward {_fmt(ratios)}")
    own = [{k: v.clone() for k, v in g.items()} for g in got]
    if c.lens is not None:
        dense = Run(c, items, dense=True)
        got_d = dense.forward()
        for m, it in enumerate(items):
            assert torch.equal(got_d[m]["out"][:it.Tq], own[m]["out"]), f"{c.name} item {m}: out of the packed call differs from the dense call"
            assert torch.equal(got_d[m]["lse"][:, :it.Tq], own[m]["lse"]), f"{c.name} item {m}: lse of the packed call differs from the dense call"
    return items, run, own, fref


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_general_fp16_forward(case):
    _run_case(case)


@pytest.mark.parametrize("one", ONEQ, ids=ONEQ_NAMES)
def test_one_query_fp16_is_row_0_of_the_full_call(one):
    name, tk, form, counts = one
    c = oneq_full_case(*one)
    items, run, full, fref = _run_case(c)
    B, H, W = c.batch, c.heads, c.heads * 64
    # the query rows: row 0 of every item.  Dense query rows of the full call: passed in place with q_ld = tq * q_ld (no copy);
    # packed ones: gathered into a dense [batch] buffer
    if run.row_off is None:
        q_ptr, q_ld = run.Q.ptr(), c.tq * run.q_ld
    else:
        Qd = Buf(B, W, W + PAD, F16)
        for m in range(B):
            Qd.view[m] = run.Q.view[run.q0[m]]
        q_ptr, q_ld = Qd.ptr(), Qd.ld
    packed = form == "packed"
    if packed and run.row_off is None:          # above 512: the item's own rows back to back, as a packed BERT holds them
        KV = Buf(sum(counts), 2 * W, run.kv_ld, F16)
        off = [sum(counts[:m]) for m in range(B + 1)]
        for m in range(B):
            KV.view[off[m]:off[m + 1]] = run.KV.view[m * tk:m * tk + counts[m]]
        kv_off = _i32(off)
    else:
        KV, kv_off = run.KV, (_i32(run.k0) if packed else None)
    key_len = None if packed else run.key_len
    out = Buf(B, W, W + PAD + 8, F16)
    lse = Buf(1, B * H, B * H + TAIL, torch.float32)
    res = []
    for _ in range(2):
        before = out.bits().clone(), lse.bits().clone()
        rc = _lib().uniir_onequery_fwd_f16(q_ptr, q_ld, KV.ptr(0), KV.ptr(W), KV.ld, out.ptr(), out.ld, lse.ptr(), _vp(key_len), _vp(kv_off),
                                           B, tk, H, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (name, rc)
        _untouched(f"{name} out", out, before[0])
        _untouched(f"{name} lse", lse, before[1])
        res.append((out.bits().clone(), lse.bits().clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), f"{name}: two calls differ"
    ratios = {}
    for m in range(B):
        o, l = out.view[m].reshape(1, H, 64), lse.view[0].view(B, H)[m].reshape(H, 1)
        assert torch.equal(o, full[m]["out"][:1]), f"{name} item {m}: out is not row 0 of the full call"
        assert torch.equal(l, full[m]["lse"][:, :1]), f"{name} item {m}: lse is not row 0 of the full call"
        for key, g in (("out", o), ("lse", l)):
            r, b = fref[m][key]
            r, b = (r[:1], b[:1]) if key == "out" else (r[:, :1], b[:, :1])
            why = R.compare(g, r, b)
            ratios[key] = max(ratios.get(key, 0.0), R.worst(g, r, b))
            assert why is None, f"{name} item {m} {key}: {why}"
    print(f"OBS {name} one-query forward {_fmt(ratios)}")


@pytest.mark.parametrize("T", [17, 33, 512, 577])
def test_the_thirds_of_a_packed_buffer_against_uniir_attention_fwd_f16(T):
    """tq == tk, no key_len, Q / K / V the thirds of one [q | k | v] buffer: up to 512 the kernel of uniir_attention_fwd_f16, the same
    bits; above, the streaming general kernel next to the plain streaming kernel: both inside the bound, agreement printed"""
    c = Case(f"thirds-{T}", "attn_fwd_kernel<0,0,1>" if T <= 512 else "attn_xlong_fwd_kernel<0,1> | attn_long_fwd_kernel<1>", "f16", 2, 2, T)
    items = R.build_items(c, DEV)
    B, H, W = c.batch, c.heads, c.heads * 64
    X = Buf(B * T, 3 * W, 3 * W, F16)
    for m, it in enumerate(items):
        rows = X.view[m * T:(m + 1) * T]
        rows[:, :W], rows[:, W:2 * W], rows[:, 2 * W:] = it.q.reshape(T, W), it.k.reshape(T, W), it.v.reshape(T, W)
    outs = []
    for general in (True, False):
        out, lse = Buf(B * T, W, W, F16), Buf(1, B * H * T, B * H * T + TAIL, torch.float32)
        before = out.bits().clone(), lse.bits().clone()
        if general:
            rc = _lib().uniir_attn_general_fwd_f16(X.ptr(0), 3 * W, X.ptr(W), X.ptr(2 * W), 3 * W, out.ptr(), W, lse.ptr(), None, 0, None,
                                                   B, T, T, H, _stream())
        else:
            rc = _lib().uniir_attention_fwd_f16(X.ptr(0), out.ptr(), lse.ptr(), None, B, T, H, 0, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, general, rc)
        _untouched(f"{c.name} out", out, before[0])
        _untouched(f"{c.name} lse", lse, before[1])
        got = [{"out": out.view[m * T:(m + 1) * T].reshape(T, H, 64), "lse": lse.view[0].view(B, H, T)[m]} for m in range(B)]
        ratios = {}
        _judge(c, "general" if general else "fwd_f16", got, [it.fwd_ref()[0] for it in items], ratios)
        outs.append((out.view.clone(), lse.view.clone()))
        print(f"OBS {c.name} {'uniir_attn_general_fwd_f16' if general else 'uniir_attention_fwd_f16'} {_fmt(ratios)}")
    same = torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    print(f"OBS {c.name} bits agree: {same}")
    if T <= 512:
        assert same, f"{c.name}: the general form and uniir_attention_fwd_f16 run one kernel and must give the same bits"


def test_the_wrappers_route_like_the_entry_point():
    """ops.attention_fwd_ex_f16 / ops.onequery_fwd_f16 on torch tensors: dense, packed query rows and the one-query form give the bits
    of each other (row 0), in the dtypes the model relies on"""
    from uniir_amd import ops
    c = CASES[NAMES.index("rows-kv0-20x40")]
    items = R.build_items(c, DEV)
    B, H, W = c.batch, c.heads, c.heads * 64
    q = torch.stack([it.twin[0] for it in items]).reshape(B * c.tq, W).contiguous()
    kv = torch.cat([torch.stack([it.twin[1] for it in items]).reshape(B * c.tk, W),
                    torch.stack([it.twin[2] for it in items]).reshape(B * c.tk, W)], 1).contiguous()
    kl = _i32(c.key_len)
    out, lse = ops.attention_fwd_ex_f16(q, W, kv, kv[:, W:], 2 * W, B, c.tq, c.tk, H, key_len=kl)
    assert out.dtype == F16 and lse.dtype == torch.float32 and out.shape == (B * c.tq, W) and lse.shape == (B, H, c.tq)
    off = [0]
    for n in c.lens:
        off.append(off[-1] + n)
    qp = torch.cat([q[m * c.tq:m * c.tq + n] for m, n in enumerate(c.lens)]).contiguous()
    outp, lsep = ops.attention_fwd_ex_f16(qp, W, kv, kv[:, W:], 2 * W, B, c.tq, c.tk, H, key_len=kl, row_off=_i32(off), kv_packed=False,
                                          rows=off[-1])
    o1, l1 = ops.onequery_fwd_f16(q, c.tq * W, kv, kv[:, W:], 2 * W, B, c.tk, H, key_len=kl)
    torch.cuda.synchronize()
    assert o1.dtype == F16 and o1.shape == (B, W) and l1.shape == (B, H)
    for m, n in enumerate(c.lens):
        assert torch.equal(outp[off[m]:off[m + 1]], out[m * c.tq:m * c.tq + n]) and torch.equal(lsep[m, :, :n], lse[m, :, :n])
        assert torch.equal(o1[m], out[m * c.tq]) and torch.equal(l1[m], lse[m, :, 0])
