"""The tower glue kernels (csrc/elementwise.hip, uniir_vit_assemble_f32, uniir_pool_inv_norms) on every path against tests/glue_ref.py.

The case tables are tests/glue_cases.py's (tests/test_glue_ref.py asserts on the CPU that every case reaches the path it names and
that every grid-stride case strides with a ragged tail).  What is compared how:
  bit for bit   patchify, vit_assemble{,_f32}, vit_assemble_bwd (dpatch, and dpos / dclass as the ascending chain onto non-zero prior
                contents), text_embed{,_packed} with eot / last_row, the position gradients of text_embed_bwd{,_packed}, gather_rows,
                scatter_rows, cast_pad_rows{,_f16}, unpad_add, cast_bf16_to_f32, the dropout masks and every dropout form,
                pool_inv_norms (the pinned chain of oracle.c), and the 16-bit conversions against torch's CPU cast on inputs built
                from all 65536 target bit patterns (value, tie, tie -/+ one fp32 ulp)
  twice         colsum_bf16 and the token gradient: integer data (bit for bit in every form, the atomic ones included), then randn
                against the fp64 sum with gamma(depth) of the form's summation tree
  bounded       act_fwd on all 65536 bf16 inputs for the three activations, tanh_fwd, tanh_bwd
Paths: the token gradient's bucket / bucket-k (kmax > 0, no long id) / bucket-long / atomic forms, dense and packed, with bucket sizes
1 .. 4097, a long id across rows 4095 / 4096, every vocabulary edge, clamped ids and the five refusals; colsum's one-block, float4
reduce, one-column reduce and atomic forms.  uniir_reduce_stats confirms each: the fallback count moves by exactly the predicted
amount and max_request equals the predicted scratch bytes; the fixed-order forms are run twice and give the same bits.  Every
grid-stride kernel runs once with work just above cap x 256 and a ragged tail.  Every tensor sits in a NaN-patterned buffer with
guard rows (fp32_cases.Buf); everything outside the logical extent keeps its bits, and a refused or empty call writes nothing.

Measured on an MI355X (the OBS lines of this file; worst |got - ref| / bound, a correct kernel stays at 0.5 or below):
  dtok      bucket forms 0.02 .. 0.31 (long-w260 dense 0.306), atomic forms 0.18 .. 0.31; every integer run bit for bit
  colsum    one row block 0.008 .. 0.026, stored partials (both reduces) and atomics at most 0.003; every integer run bit for bit
  act_fwd   QuickGELU 0.498, erf-GELU 0.486 -- the bf16 rounding of the result itself (the fp32 restatement of
            tests/test_glue_ref.py sits at the same figures), ReLU 0
  tanh      forward 0.074, backward 0.365
  casts     all 1028 (bf16) and 6 (fp16) inputs in fp32's subnormal range came out as the IEEE result, from the packed convert of
            cast_f32_to_* and from the scalar convert of cast_pad_rows*: nothing is flushed
  resid + x * m (dropout_f32, dense and packed rows): every element equals the two-rounding form; the 25 % or so that differ from
            the fused form show that the build does not contract this one
One defect was found while the references were written and is fixed with this file: act_fwd's ReLU was fmaxf(x, 0), which returns 0
for a NaN; it now hands the NaN on (test_act_fwd_every_bf16_value[relu]).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fp32_cases as F32
import glue_cases as T
import glue_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16 = torch.bfloat16, torch.float16
OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
Buf = F32.Buf


def _lib():
    from uniir_amd import _lib
    return _lib.load()


def _st():
    from uniir_amd import ops
    return ops._stream()


def _p(b):
    if b is None:
        return None
    return C.c_void_p(b.view.data_ptr() if isinstance(b, Buf) else b.data_ptr())


def _buf(t, ld=None, off=0, dtype=None):
    t = t if t.dim() == 2 else t.reshape(1, -1)
    return Buf(t.shape[0], t.shape[1], ld, dtype=dtype or t.dtype, off=off, device=DEV).set(t.to(DEV))


def _out(rows, cols, ld=None, dtype=torch.float32, off=0):
    return Buf(rows, cols, ld, dtype=dtype, off=off, device=DEV)


def _call(name, outs, *args, rc=OK):
    """one checked call: the return code, and every output unchanged outside its extent (everywhere, if the call is refused)"""
    before = [b.bits().clone() for b in outs]
    got = getattr(_lib(), name)(*args, _st())
    torch.cuda.synchronize()
    assert got == rc, (name, got, rc)
    for b, was in zip(outs, before):
        if rc == OK:
            b.assert_outside_untouched(was, name)
        else:
            b.assert_all_untouched(was, name)


def _stats(reset=False):
    f, m = C.c_int64(), C.c_int64()
    assert _lib().uniir_reduce_stats(C.byref(f), C.byref(m), 1 if reset else 0) == 0
    return f.value, m.value


class _Scratch:
    """the stream's reduction scratch for one call: ops' buffer ("on"), none ("off") or a temporary one of `bytes`"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from uniir_amd import ops
        self.lib = _lib()
        self.stream = ops._stream()
        s = torch.cuda.current_stream()
        self.keep = ops._RED_SCRATCH[(s.device.index, s.cuda_stream)]
        if self.mode == "off":
            assert self.lib.uniir_reduce_scratch(None, 0, self.stream) == 0
        elif self.mode != "on":
            self.tmp = torch.empty(int(self.mode), dtype=torch.uint8, device=DEV)
            assert self.lib.uniir_reduce_scratch(C.c_void_p(self.tmp.data_ptr()), int(self.mode), self.stream) == 0
        return self.stream

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        if self.mode != "on":
            assert self.lib.uniir_reduce_scratch(C.c_void_p(self.keep.data_ptr()), self.keep.numel(), self.stream) == 0
        return False


def _counted(plan, scratch, fn):
    """run fn under the scratch mode of the case and hold uniir_reduce_stats to the plan: fallbacks and the bytes asked for"""
    _st()
    torch.cuda.synchronize()
    _stats(reset=True)
    mode = scratch if scratch != "short" else plan["bytes"] - 1
    try:
        with _Scratch(mode) as st:
            rc = fn(st)
        assert rc == OK, rc
        f, m = _stats()
        assert f == plan["fallbacks"], f"fallbacks moved by {f}, predicted {plan['fallbacks']} ({plan})"
        assert m == plan["bytes"], f"max_request {m}, predicted {plan['bytes']} ({plan})"
    finally:
        _stats(reset=True)


def _obs(name, **kw):
    print(f"\nOBS {name}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in kw.items()))


def _rand(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape)))


# ======================================================================================================================= patchify
@pytest.mark.parametrize("name,n,res,P,kpad", T.PATCHIFY + [T.PATCHIFY_BIG], ids=[c[0] for c in T.PATCHIFY + [T.PATCHIFY_BIG]])
def test_patchify(name, n, res, P, kpad):
    img = torch.randn(n, 3, res, res, device=DEV, generator=torch.Generator(device=DEV).manual_seed(res))
    g = res // P
    out = _out(n * g * g, kpad, dtype=BF16)
    _call("uniir_patchify", [out], _p(img), _p(out), n, res, P, kpad)
    G.assert_bits(out.view, G.patchify(img, P, kpad), name)


# =================================================================================================================== vit_assemble
@pytest.mark.parametrize("n,T_,w", T.ASSEMBLE + [T.ASSEMBLE_BIG], ids=lambda v: str(v))
def test_vit_assemble(n, T_, w):
    g = torch.Generator(device=DEV).manual_seed(w + T_)
    po = torch.randn(n * (T_ - 1), w, device=DEV, generator=g).to(BF16)
    cls, pos = torch.randn(w, device=DEV, generator=g), torch.randn(T_, w, device=DEV, generator=g)
    x = _out(n * T_, w)
    _call("uniir_vit_assemble", [x], _p(po), _p(cls), _p(pos), _p(x), n, T_, w)
    G.assert_bits(x.view, G.vit_assemble(po, cls, pos, n, T_), "vit_assemble")


@pytest.mark.parametrize("n,T_,w", T.ASSEMBLE + [T.ASSEMBLE_F32_BIG], ids=lambda v: str(v))
def test_vit_assemble_f32(n, T_, w):
    g = torch.Generator(device=DEV).manual_seed(w + T_)
    po, cls, pos = (torch.randn(*s, device=DEV, generator=g) for s in ((n * (T_ - 1), w), (w,), (T_, w)))
    x = _out(n * T_, w)
    _call("uniir_vit_assemble_f32", [x], _p(po), _p(cls), _p(pos), _p(x), n, T_, w)
    G.assert_bits(x.view, G.vit_assemble(po, cls, pos, n, T_), "vit_assemble_f32")


@pytest.mark.parametrize("n,T_,w", T.ASSEMBLE, ids=lambda v: str(v))
def test_vit_assemble_bwd(n, T_, w):
    dx = _buf(_rand(n * T_, w))
    dpatch = _out(n * (T_ - 1), w, dtype=BF16)
    dclass, dpos = _buf(_rand(1, w, seed=1)), _buf(_rand(T_, w, seed=2))
    ref = G.vit_assemble_bwd(dx.view.clone(), n, T_, dclass.view[0].clone(), dpos.view.clone())
    _call("uniir_vit_assemble_bwd", [dpatch, dclass, dpos], _p(dx), _p(dpatch), _p(dclass), _p(dpos), n, T_, w)
    G.assert_bits(dpatch.view, ref["dpatch"], "dpatch")
    G.assert_bits(dpos.view, ref["dpos"], "dpos")
    G.assert_bits(dclass.view[0], ref["dclass"], "dclass")


# ===================================================================================================================== text_embed
def _text_ids(n, ctx, vocab, oob):
    g = torch.Generator().manual_seed(vocab + n)
    text = torch.randint(-3 if oob else 0, vocab + (3 if oob else 0), (n, ctx), generator=g).to(torch.int32)
    text[0, 0] = -2 if oob else 0
    text[-1, -1] = vocab + 1 if oob else vocab - 1
    if n > 1 and ctx > 2:
        text[1, :] = text[1, 0]                       # a row of equal ids: the first arg-max is 0
        text[-1, 1] = text[-1, -1]                    # the maximum twice
    return text.to(DEV)


@pytest.mark.parametrize("n,ctx,w,vocab,oob", T.TEXT + [T.TEXT_BIG + (True,)], ids=lambda v: str(v))
def test_text_embed(n, ctx, w, vocab, oob):
    g = torch.Generator(device=DEV).manual_seed(vocab)
    text = _text_ids(n, ctx, vocab, oob)
    tok, pos = torch.randn(vocab, w, device=DEV, generator=g), torch.randn(ctx, w, device=DEV, generator=g)
    x, eot = _out(n * ctx, w), _out(1, n, n + 64, dtype=torch.int32)
    _call("uniir_text_embed", [x, eot], _p(text), _p(tok), _p(pos), _p(x), _p(eot), n, ctx, w, vocab)
    want, want_eot = G.text_embed(text, tok, pos, vocab)
    G.assert_bits(x.view, want, "text_embed")
    assert torch.equal(eot.view[0].cpu(), want_eot), "eot"
    x2 = _out(n * ctx, w)                             # eot may be NULL
    _call("uniir_text_embed", [x2], _p(text), _p(tok), _p(pos), _p(x2), None, n, ctx, w, vocab)
    assert torch.equal(x2.bits(), x.bits())
    # packed: lengths 1 .. ctx, 1 and ctx among them
    lens = torch.randint(1, ctx + 1, (n,), generator=torch.Generator().manual_seed(n)).to(torch.int32)
    lens[0], lens[-1] = ctx, 1 if n > 1 else ctx
    lens = lens.to(DEV)
    off = G.row_offsets(lens)
    total = int(off[-1])
    xp, last = _out(total, w), _out(1, n, n + 64, dtype=torch.int32)
    _call("uniir_text_embed_packed", [xp, last], _p(text), _p(tok), _p(pos), _p(off), _p(xp), _p(last), n, ctx, w, vocab)
    want, want_last = G.text_embed_packed(text, tok, pos, vocab, lens)
    G.assert_bits(xp.view, want, "text_embed_packed")
    assert torch.equal(last.view[0], want_last), "last_row"
    xp2 = _out(total, w)                              # last_row may be NULL
    _call("uniir_text_embed_packed", [xp2], _p(text), _p(tok), _p(pos), _p(off), _p(xp2), None, n, ctx, w, vocab)
    assert torch.equal(xp2.bits(), xp.bits())


# ================================================================================================================= token gradient
class _Tok:
    def __init__(self, c, packed, integer):
        self.c, self.packed = c, packed
        self.lens = T.tok_lens(c) if packed else None
        self.text = T.tok_text(c, lens=self.lens)
        rows = int(self.lens.sum()) if packed else c.rows
        self.cnt = G.token_counts(self.text, c.vocab, self.lens)
        self.plan = T.tok_plan(c, c.rows, int(self.cnt.max()))
        self.dx_cpu, self.dtok0, self.dpos0 = T.tok_data(c, rows, integer)
        self.text_d = self.text.to(DEV)
        self.off_d = G.row_offsets(self.lens).to(DEV) if packed else None
        self.dx = _buf(self.dx_cpu, off=c.dx_off)
        self.fresh()

    def fresh(self):
        self.dtok, self.dpos = _buf(self.dtok0, off=self.c.dtok_off), _buf(self.dpos0)

    def call(self, st):
        c, lib = self.c, _lib()
        if self.packed:
            return lib.uniir_text_embed_bwd_packed(_p(self.text_d), _p(self.dx), _p(self.off_d), _p(self.dtok), _p(self.dpos), c.n,
                                                   c.ctx, c.w, c.vocab, st)
        return lib.uniir_text_embed_bwd(_p(self.text_d), _p(self.dx), _p(self.dtok), _p(self.dpos), c.n, c.ctx, c.w, c.vocab, st)

    def run(self):
        before = [b.bits().clone() for b in (self.dtok, self.dpos)]
        _counted(self.plan, self.c.scratch, self.call)
        for b, was in zip((self.dtok, self.dpos), before):
            b.assert_outside_untouched(was, self.c.name)
        return self.dtok.view.cpu(), self.dpos.view.cpu()


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("c", T.TOK, ids=[c.name for c in T.TOK])
def test_token_gradient(c, packed):
    ratios = {}
    for integer in (True, False):
        t = _Tok(c, packed, integer)
        assert t.plan["form"] == c.path
        dtok, dpos = t.run()
        fixed = c.path != "atomic"
        ref, bound = G.dtok(t.text, t.dx_cpu, c.vocab, t.dtok0, fixed, t.lens, t.plan["nslices"])
        G.check(dtok, ref, bound, f"{c.name} dtok ({'integers' if integer else 'randn'})")
        if integer:
            assert float(bound.max()) == 0.0
        else:
            ratios["dtok"] = G.worst_ratio(dtok, ref, bound)
        G.assert_bits(dpos, G.text_dpos(t.dx_cpu, c.n, c.ctx, t.dpos0, t.lens), f"{c.name} dpos")
        if fixed:                                     # the same bits on a second run, and still nothing counted
            t.fresh()
            again, _ = t.run()
            G.assert_bits(again, dtok, f"{c.name}: two runs")
    _obs(f"dtok {c.name} {'packed' if packed else 'dense'} {c.path}", **ratios)


# ========================================================================================================================= colsum
@pytest.mark.parametrize("c", T.COLSUM, ids=[c.name for c in T.COLSUM])
def test_colsum(c):
    plan = T.colsum_plan(c.rows, c.cols, c.out_off % 4 == 0, c.scratch)
    assert plan["form"] == c.path
    depth = G.colsum_depth(plan["rpb"], plan["gy"])
    ratios = {}
    for integer in (True, False):
        x_cpu, out0 = T.colsum_data(c, integer)
        x = _buf(x_cpu, ld=c.cols + c.pad)
        got = []
        for _ in range(2 if c.path != "atomic" else 1):
            out = _buf(out0, ld=c.cols + 64, off=c.out_off)
            was = out.bits().clone()
            _counted(plan, c.scratch, lambda st: _lib().uniir_colsum_bf16(_p(x), c.cols + c.pad, _p(out), c.rows, c.cols, st))
            out.assert_outside_untouched(was, c.name)
            got.append(out.view[0].cpu())
        ref, bound = G.colsum(x_cpu, out0, depth)
        G.check(got[0], ref, bound, f"{c.name} ({'integers' if integer else 'randn'})")
        if integer:
            assert float(bound.max()) == 0.0
        else:
            ratios["colsum"] = G.worst_ratio(got[0], ref, bound)
        if len(got) == 2:
            G.assert_bits(got[1], got[0], f"{c.name}: two runs")
    _obs(f"colsum {c.name} {c.path}", **ratios)


# ================================================================================================================ gather / scatter
@pytest.mark.parametrize("n,seq,w,kind", T.GATHER + [T.GATHER_BIG], ids=lambda v: str(v))
def test_gather_scatter_rows(n, seq, w, kind):
    total = n * seq if seq else 3 * n
    g = torch.Generator(device=DEV).manual_seed(n)
    x0, dout = torch.randn(total, w, device=DEV, generator=g), torch.randn(n, w, device=DEV, generator=g)
    idx = T.gather_idx(n, seq, kind, total, DEV)
    out = _out(n, w)
    _call("uniir_gather_rows", [out], _p(x0), _p(idx), _p(out), n, seq, w)
    G.assert_bits(out.view, G.gather_rows(x0, idx, n, seq), "gather_rows")
    dx = _buf(x0)
    _call("uniir_scatter_rows", [dx], _p(dout), _p(idx), _p(dx), n, seq, w)
    G.assert_bits(dx.view, G.scatter_rows(dout, idx, x0, seq), "scatter_rows")          # the rows not indexed keep their bits


# ==================================================================================================================== activations
def _tile(t, count):
    return t.repeat(-(-count // t.numel()))[:count].contiguous()


@pytest.mark.parametrize("act", [G.QUICK_GELU, G.ERF_GELU, G.RELU], ids=["quickgelu", "erfgelu", "relu"])
def test_act_fwd_every_bf16_value(act):
    x = T.all_bf16(DEV)
    out = _out(1, 65536, dtype=BF16)
    _call("uniir_act_fwd", [out], _p(x), _p(out), 65536, act)
    got, xf = out.view[0].cpu(), x.float().cpu()
    fin = torch.isfinite(xf)
    ref, bound = G.act_fwd(xf[fin], act)
    G.check(got[fin], ref, bound, f"act {act}")
    _obs(f"act_fwd act {act}", worst=G.worst_ratio(got[fin], ref, bound))
    sp, gs = G.act_special(xf[~fin], act), got[~fin].double()
    assert torch.equal(torch.isnan(sp), torch.isnan(gs)), "NaN in gives NaN out; infinities follow the fp64 formula"
    assert torch.equal(sp[~torch.isnan(sp)], gs[~torch.isnan(gs)])
    # the grid-stride loop: every element of a long call equals the element of the short one
    big = _tile(x, T.ACT_BIG)
    obig = _out(1, T.ACT_BIG, dtype=BF16)
    _call("uniir_act_fwd", [obig], _p(big), _p(obig), T.ACT_BIG, act)
    want = _tile(out.view[0], T.ACT_BIG)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(obig.view[0]), nan) and torch.equal(obig.view[0][~nan].view(torch.int16), want[~nan].view(torch.int16))


def test_tanh():
    for n in (4099, T.TANH_BIG):
        x_cpu, dy_cpu = T.tanh_data(n)
        x, dy = x_cpu.to(DEV), dy_cpu.to(DEV)
        y, dx = _out(1, n), _out(1, n)
        _call("uniir_tanh_fwd", [y], _p(x), _p(y), n)
        ref, bound = G.tanh_fwd(x_cpu)
        G.check(y.view[0].cpu(), ref, bound, f"tanh_fwd {n}")
        r_f = G.worst_ratio(y.view[0].cpu(), ref, bound)
        _call("uniir_tanh_bwd", [dx], _p(y), _p(dy), _p(dx), n)
        ref, bound = G.tanh_bwd(y.view[0].cpu(), dy_cpu)
        G.check(dx.view[0].cpu(), ref, bound, f"tanh_bwd {n}")
        _obs(f"tanh n={n}", fwd=r_f, bwd=G.worst_ratio(dx.view[0].cpu(), ref, bound))
    sp = torch.tensor([float("inf"), float("-inf"), float("nan"), 0.0], device=DEV)
    y = _out(1, 4)
    _call("uniir_tanh_fwd", [y], _p(sp), _p(y), 4)
    got = y.view[0].cpu()
    assert got[0] == 1.0 and got[1] == -1.0 and bool(torch.isnan(got[2])) and got[3] == 0.0
    one = torch.tensor([1.0, -1.0], device=DEV)
    dx = _out(1, 2)
    _call("uniir_tanh_bwd", [dx], _p(one), _p(one), _p(dx), 2)
    assert bool((dx.view[0] == 0).all())


# ==================================================================================================================== conversions
CASTS = {BF16: "uniir_cast_f32_to_bf16", F16: "uniir_cast_f32_to_f16"}


def _verdict(x_cpu, got, dt, what):
    bad, nsub, ieee, zero = G.cast_verdict(x_cpu, got, dt)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} conversions wrong; first input {float(x_cpu[i])!r} "
                             f"({int(x_cpu.view(torch.int32)[i]) & 0xffffffff:#x}) -> {int(G.ibits(got.cpu())[i]) & 0xffff:#x}")
    return nsub, ieee, zero


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_cast_every_target_value(dt):
    x_cpu = G.cast_inputs(dt)
    n = x_cpu.numel()
    x = x_cpu.to(DEV)
    out = _out(1, n, n + 64, dtype=dt)
    _call(CASTS[dt], [out], _p(x), _p(out), n)
    nsub, ieee, zero = _verdict(x_cpu, out.view[0], dt, CASTS[dt])
    cols = 1003                                        # the scalar convert of cast_pad_rows on the same inputs
    rows = -(-n // cols)
    xp_cpu = torch.cat([x_cpu, torch.zeros(rows * cols - n)])
    pad, xp = _out(rows, cols + 5, dtype=dt), xp_cpu.to(DEV)
    name = "uniir_cast_pad_rows" if dt == BF16 else "uniir_cast_pad_rows_f16"
    _call(name, [pad], _p(xp), _p(pad), rows, cols, cols + 5)
    s2 = _verdict(xp_cpu, pad.view[:, :cols].reshape(-1), dt, name)
    assert bool((pad.view[:, cols:].view(torch.int16) == 0).all())
    _obs(f"cast to {dt}", subnormal_inputs=nsub, ieee=ieee, flushed_to_zero=zero, pad_rows_ieee=s2[1], pad_rows_flushed=s2[2])
    # the grid-stride loop with a live tail: a long call equals the short one element by element
    big = _tile(x, T.CAST_BIG)
    obig = _out(1, T.CAST_BIG, T.CAST_BIG + 64, dtype=dt)
    _call(CASTS[dt], [obig], _p(big), _p(obig), T.CAST_BIG)
    want, got = _tile(out.view[0], T.CAST_BIG), obig.view[0]
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16))


@pytest.mark.parametrize("count", T.CAST_COUNTS)
def test_cast_counts(count):
    x_cpu = _rand(count) * 100.0
    x = x_cpu.to(DEV)
    for dt in (BF16, F16):
        out = _out(1, count, count + 64, dtype=dt)
        _call(CASTS[dt], [out], _p(x), _p(out), count)
        G.assert_bits(out.view[0], x_cpu.to(dt), f"{CASTS[dt]} count {count}")
    b = x_cpu.to(BF16).to(DEV)
    f = _out(1, count, count + 64)
    _call("uniir_cast_bf16_to_f32", [f], _p(b), _p(f), count)
    G.assert_bits(f.view[0], G.bf16_to_f32(b), f"bf16_to_f32 count {count}")


def test_cast_bf16_to_f32_every_value_and_strided():
    b = T.all_bf16(DEV)
    f = _out(1, 65536)
    _call("uniir_cast_bf16_to_f32", [f], _p(b), _p(f), 65536)
    G.assert_bits(f.view[0], G.bf16_to_f32(b), "bf16_to_f32")
    big = _tile(b, T.BF16_F32_BIG)
    f = _out(1, T.BF16_F32_BIG)
    _call("uniir_cast_bf16_to_f32", [f], _p(big), _p(f), T.BF16_F32_BIG)
    G.assert_bits(f.view[0], G.bf16_to_f32(big), "bf16_to_f32 strided")


@pytest.mark.parametrize("rows,cols,ld", T.PAD_ROWS + [T.PAD_ROWS_BIG], ids=lambda v: str(v))
def test_cast_pad_rows(rows, cols, ld):
    src = torch.randn(rows, cols, device=DEV, generator=torch.Generator(device=DEV).manual_seed(ld))
    for name, dt in (("uniir_cast_pad_rows", BF16), ("uniir_cast_pad_rows_f16", F16)):
        dst = _out(rows, ld, dtype=dt)
        _call(name, [dst], _p(src), _p(dst), rows, cols, ld)
        G.assert_bits(dst.view, G.cast_pad_rows(src, ld, dt), name)


@pytest.mark.parametrize("rows,cols,ld", T.PAD_ROWS + [T.UNPAD_BIG], ids=lambda v: str(v))
def test_unpad_add(rows, cols, ld):
    g = torch.Generator(device=DEV).manual_seed(ld)
    src = _buf(torch.randn(rows, cols, device=DEV, generator=g), ld=ld)          # NaN pattern between cols and ld
    dst0 = torch.randn(rows, cols, device=DEV, generator=g)
    dst = _buf(dst0)
    _call("uniir_unpad_add", [dst], _p(src), _p(dst), rows, cols, ld)
    G.assert_bits(dst.view, dst0 + src.view, "unpad_add")


# ======================================================================================================================== dropout
def _mask_call(count, p, seed):
    out = _out(1, count)
    _call("uniir_dropout_mask", [out], _p(out), count, p, seed)
    return out.view[0]


def _f32_form(c, x, resid, rowscale, row_map, factor, split):
    """uniir_dropout_f32 (or _rows with row_map) in the output combination of the case against the accepted forms"""
    y32 = _out(c.rows, c.cols) if c.outs in ("f32", "both") else None
    y16 = _out(c.rows, c.cols, dtype=BF16) if c.outs in ("bf16", "both") else None
    outs = [b for b in (y32, y16) if b is not None]
    r = resid if c.resid else None
    if row_map is None:
        _call("uniir_dropout_f32", outs, _p(x), _p(r), _p(y32), _p(y16), c.rows, c.cols, c.p, c.seed, _p(rowscale), c.div)
    else:
        _call("uniir_dropout_f32_rows", outs, _p(x), _p(r), _p(y32), _p(y16), c.rows, c.cols, c.p, c.seed, _p(row_map))
    forms = G.dropout_forms(x.cpu().numpy(), factor, r.cpu().numpy() if c.resid else None)
    if y32 is not None:
        ok, two, fused, both = G.dropout_accepts(y32.view.cpu().numpy(), forms)
        assert ok.all(), f"{c.name}: {int((~ok).sum())} elements are neither resid + fl(x m) nor fma(x, m, resid)"
        for k, v in (("two_roundings_only", two), ("fused_only", fused), ("either", both)):
            split[k] = split.get(k, 0) + v
        if y16 is not None:
            G.assert_bits(y16.view, y32.view.to(BF16), f"{c.name}: the bf16 copy is the fp32 result rounded")
    else:
        ok, _, _, _ = G.dropout_accepts(y16.view.view(torch.int16).cpu().numpy().view(np.uint16), forms, bf16=True)
        assert ok.all(), f"{c.name}: {int((~ok).sum())} bf16 elements match neither form"
    return y32, y16


@pytest.mark.parametrize("c", T.DROP + [T.DROP_BIG], ids=[c.name for c in T.DROP + [T.DROP_BIG]])
def test_dropout(c):
    x, resid, rowscale, row_map = T.drop_data(c, DEV)
    split = {}
    mask = G.drop_mask(c.rows, c.cols, c.p, c.seed)
    factor = G.drop_factor(mask, None if rowscale is None else rowscale.cpu().numpy(), c.div or 1)
    if c is not T.DROP_BIG:                               # (the strided mask call has its own count below)
        G.assert_bits(_mask_call(c.rows * c.cols, c.p, c.seed), torch.from_numpy(G.drop_mask(c.rows, c.cols, c.p, c.seed,
                                                                                              always_hash=True)).flatten(), "mask")
    _f32_form(c, x, resid, rowscale, None, factor, split)
    # bf16 -> bf16 with a pitch: the padding keeps its pattern, the mask index has no pitch in it
    xb = _buf(x.to(BF16), ld=c.cols + c.pad)
    yb = _out(c.rows, c.cols, c.cols + c.pad, dtype=BF16)
    _call("uniir_dropout_bf16", [yb], _p(xb), _p(yb), c.rows, c.cols, c.cols + c.pad, c.p, c.seed, _p(rowscale), c.div)
    G.assert_bits(yb.view, G.dropout_bf16(xb.view, factor), f"{c.name} dropout_bf16")
    # the packed forms: row r is row row_map[r] of the logical tensor
    rm = row_map.cpu().numpy()
    pmask = G.drop_mask(c.rows, c.cols, c.p, c.seed, rm)
    y32, y16 = _f32_form(c, x, resid, None, row_map, pmask, split)
    ybr = _out(c.rows, c.cols, c.cols + c.pad, dtype=BF16)
    _call("uniir_dropout_bf16_rows", [ybr], _p(xb), _p(ybr), c.rows, c.cols, c.cols + c.pad, c.p, c.seed, _p(row_map))
    G.assert_bits(ybr.view, G.dropout_bf16(xb.view, pmask), f"{c.name} dropout_bf16_rows")
    if c is not T.DROP_BIG:
        # ... and bit for bit the mapped rows of the dense call on the logical tensor at the same seed
        R_ = 2 * c.rows + 3
        lx, lres = torch.zeros(R_, c.cols, device=DEV), torch.zeros(R_, c.cols, device=DEV)
        lx[row_map.long()], lres[row_map.long()] = x, resid
        d32 = _out(R_, c.cols) if y32 is not None else None
        d16 = _out(R_, c.cols, dtype=BF16) if y16 is not None else None
        _call("uniir_dropout_f32", [b for b in (d32, d16) if b is not None], _p(lx), _p(lres if c.resid else None), _p(d32), _p(d16),
              R_, c.cols, c.p, c.seed, None, 0)
        for packed, dense in ((y32, d32), (y16, d16)):
            if packed is not None:
                G.assert_bits(packed.view, dense.view[row_map.long()], f"{c.name}: rows form against the dense call")
        lb = _buf(lx.to(BF16), ld=c.cols + c.pad)
        lb.view[row_map.long()] = xb.view
        db = _out(R_, c.cols, c.cols + c.pad, dtype=BF16)
        _call("uniir_dropout_bf16", [db], _p(lb), _p(db), R_, c.cols, c.cols + c.pad, c.p, c.seed, None, 0)
        G.assert_bits(ybr.view, db.view[row_map.long()], f"{c.name}: bf16 rows form against the dense call")
    _obs(f"dropout {c.name} resid + x m", **split)


def test_dropout_mask_strided():
    n = T.DROP_MASK_BIG
    want = torch.from_numpy(G.drop_mask(1, n, 0.1, 99, always_hash=True)).flatten()
    G.assert_bits(_mask_call(n, 0.1, 99), want, "dropout_mask")


# ================================================================================================================= pool_inv_norms
@pytest.mark.parametrize("n,dim", T.INV_NORMS)
def test_pool_inv_norms(n, dim):
    x = T.inv_norm_data(n, dim, DEV)
    inv = _out(1, n, n + 64)
    _call("uniir_pool_inv_norms", [inv], _p(x), n, dim, _p(inv))
    G.assert_bits(inv.view[0], G.inv_norms(x), "pool_inv_norms")
    assert float(inv.view[0][n // 2]) == 0.0


# ======================================================================================================================= refusals
def test_refusals_write_nothing():
    """every EINVAL / ESHAPE / EALIGN the host entries check returns its code and leaves every output's bits; n == 0 / count == 0
    return OK and write nothing"""
    lib, st = _lib(), _st()
    f32, b16 = _buf(_rand(64, 64)), _buf(_rand(64, 64), dtype=BF16)          # inputs
    i32 = _buf(torch.zeros(1, 64, dtype=torch.int32))
    o32, o16, oi = _buf(_rand(64, 64, seed=5)), _buf(_rand(64, 64, seed=6), dtype=BF16), _buf(torch.ones(1, 64, dtype=torch.int32))
    o32b, o32c = _buf(_rand(64, 64, seed=7)), _buf(_rand(64, 64, seed=8))
    outs = (o32, o16, oi, o32b, o32c)
    before = [b.bits().clone() for b in outs]
    A, H, I, X, Y, Z, J = _p(f32), _p(b16), _p(i32), _p(o32), _p(o16), _p(o32b), _p(oi)
    W = _p(o32c)
    off4 = C.c_void_p(f32.view.data_ptr() + 4)
    off2 = C.c_void_p(o16.view.data_ptr() + 2)
    plan = []

    def add(code, fn, *args):
        plan.append((code, fn, args))

    for bad, code in (((None, Y, 1, 16, 16, 768), EINVAL), ((A, None, 1, 16, 16, 768), EINVAL), ((A, Y, -1, 16, 16, 768), EINVAL),
                      ((A, Y, 0, 16, 16, 768), OK), ((A, Y, 1, 16, 0, 768), ESHAPE), ((A, Y, 1, 30, 16, 768), ESHAPE),
                      ((A, Y, 1, 16, 16, 772), ESHAPE), ((A, Y, 1, 16, 16, 760), ESHAPE)):
        add(code, "uniir_patchify", *bad)
    for name, src, shape in (("uniir_vit_assemble", H, ESHAPE), ("uniir_vit_assemble_f32", A, EINVAL)):
        for bad, code in (((None, A, A, X, 1, 3, 8), EINVAL), ((src, None, A, X, 1, 3, 8), EINVAL), ((src, A, None, X, 1, 3, 8), EINVAL),
                          ((src, A, A, None, 1, 3, 8), EINVAL), ((src, A, A, X, -1, 3, 8), EINVAL), ((src, A, A, X, 0, 3, 8), OK),
                          ((src, A, A, X, 1, 1, 8), shape)):
            add(code, name, *bad)
    add(ESHAPE, "uniir_vit_assemble", H, A, A, X, 1, 3, 6)
    add(EINVAL, "uniir_vit_assemble_f32", A, A, A, X, 1, 3, 0)
    for bad, code in (((None, Y, X, Z, 1, 3, 8), EINVAL), ((A, None, X, Z, 1, 3, 8), EINVAL), ((A, Y, None, Z, 1, 3, 8), EINVAL),
                      ((A, Y, X, None, 1, 3, 8), EINVAL), ((A, Y, X, Z, -1, 3, 8), EINVAL), ((A, Y, X, Z, 0, 3, 8), OK)):
        add(code, "uniir_vit_assemble_bwd", *bad)
    for bad, code in (((None, A, A, X, J, 1, 3, 8, 4), EINVAL), ((I, None, A, X, J, 1, 3, 8, 4), EINVAL), ((I, A, None, X, J, 1, 3, 8, 4), EINVAL),
                      ((I, A, A, None, J, 1, 3, 8, 4), EINVAL), ((I, A, A, X, J, -1, 3, 8, 4), EINVAL), ((I, A, A, X, J, 0, 3, 8, 4), OK),
                      ((I, A, A, X, J, 1, 3, 6, 4), ESHAPE)):
        add(code, "uniir_text_embed", *bad)
    for bad, code in (((None, A, A, I, X, J, 1, 3, 8, 4), EINVAL), ((I, None, A, I, X, J, 1, 3, 8, 4), EINVAL),
                      ((I, A, None, I, X, J, 1, 3, 8, 4), EINVAL), ((I, A, A, None, X, J, 1, 3, 8, 4), EINVAL),
                      ((I, A, A, I, None, J, 1, 3, 8, 4), EINVAL), ((I, A, A, I, X, J, -1, 3, 8, 4), EINVAL),
                      ((I, A, A, I, X, J, 0, 3, 8, 4), OK), ((I, A, A, I, X, J, 1, 3, 6, 4), ESHAPE)):
        add(code, "uniir_text_embed_packed", *bad)
    for bad, code in (((None, A, X, Z, 1, 3, 8, 4), EINVAL), ((I, None, X, Z, 1, 3, 8, 4), EINVAL), ((I, A, None, Z, 1, 3, 8, 4), EINVAL),
                      ((I, A, X, None, 1, 3, 8, 4), EINVAL), ((I, A, X, Z, -1, 3, 8, 4), EINVAL), ((I, A, X, Z, 0, 3, 8, 4), OK)):
        add(code, "uniir_text_embed_bwd", *bad)
    for bad, code in (((None, A, I, X, Z, 1, 3, 8, 4), EINVAL), ((I, None, I, X, Z, 1, 3, 8, 4), EINVAL), ((I, A, None, X, Z, 1, 3, 8, 4), EINVAL),
                      ((I, A, I, None, Z, 1, 3, 8, 4), EINVAL), ((I, A, I, X, None, 1, 3, 8, 4), EINVAL), ((I, A, I, X, Z, -1, 3, 8, 4), EINVAL),
                      ((I, A, I, X, Z, 0, 3, 8, 4), OK)):
        add(code, "uniir_text_embed_bwd_packed", *bad)
    for name in ("uniir_gather_rows", "uniir_scatter_rows"):
        for bad, code in (((None, I, X, 2, 3, 8), EINVAL), ((A, I, None, 2, 3, 8), EINVAL), ((A, I, X, -1, 3, 8), EINVAL), ((A, I, X, 0, 3, 8), OK),
                          ((A, I, X, 2, 3, 6), ESHAPE)):
            add(code, name, *bad)
    for bad, code in (((None, Y, 8, 0), EINVAL), ((H, None, 8, 0), EINVAL), ((H, Y, -8, 0), EINVAL), ((H, Y, 0, 0), OK), ((H, Y, 12, 0), ESHAPE)):
        add(code, "uniir_act_fwd", *bad)
    for bad, code in (((None, 64, X, 4, 8), EINVAL), ((H, 64, None, 4, 8), EINVAL), ((H, 64, X, -1, 8), EINVAL), ((H, 64, X, 4, 0), EINVAL),
                      ((H, 64, X, 0, 8), OK), ((H, 64, X, 4, 12), ESHAPE), ((H, 60, X, 4, 8), ESHAPE)):
        add(code, "uniir_colsum_bf16", *bad)
    for name in CASTS.values():
        for bad, code in (((None, Y, 8), EINVAL), ((A, None, 8), EINVAL), ((A, Y, -1), EINVAL), ((A, Y, 0), OK), ((off4, Y, 8), EALIGN),
                          ((A, off2, 8), EALIGN)):
            add(code, name, *bad)
    for bad, code in (((None, X, 8), EINVAL), ((H, None, 8), EINVAL), ((H, X, -1), EINVAL), ((H, X, 0), OK)):
        add(code, "uniir_cast_bf16_to_f32", *bad)
    for name, dst in (("uniir_cast_pad_rows", Y), ("uniir_cast_pad_rows_f16", Y), ("uniir_unpad_add", X)):
        for bad, code in (((None, dst, 2, 4, 8), EINVAL), ((A, None, 2, 4, 8), EINVAL), ((A, dst, -1, 4, 8), EINVAL), ((A, dst, 2, 0, 8), EINVAL),
                          ((A, dst, 2, 8, 4), EINVAL), ((A, dst, 0, 4, 8), OK)):
            add(code, name, *bad)
    for bad, code in (((None, X, 8), EINVAL), ((A, None, 8), EINVAL), ((A, X, -1), EINVAL), ((A, X, 0), OK)):
        add(code, "uniir_tanh_fwd", *bad)
    for bad, code in (((None, A, X, 8), EINVAL), ((A, None, X, 8), EINVAL), ((A, A, None, 8), EINVAL), ((A, A, X, -1), EINVAL), ((A, A, X, 0), OK)):
        add(code, "uniir_tanh_bwd", *bad)
    S = 7
    for bad, code in (((None, A, X, Y, 2, 8, 0.1, S, None, 0), EINVAL), ((A, A, None, None, 2, 8, 0.1, S, None, 0), EINVAL),
                      ((A, A, X, Y, -1, 8, 0.1, S, None, 0), EINVAL), ((A, A, X, Y, 2, 0, 0.1, S, None, 0), EINVAL),
                      ((A, A, X, Y, 2, 6, 0.1, S, None, 0), EINVAL), ((A, A, X, Y, 2, 8, -0.1, S, None, 0), EINVAL),
                      ((A, A, X, Y, 2, 8, 1.0, S, None, 0), EINVAL), ((A, A, X, Y, 2, 8, 0.1, S, A, 0), EINVAL),
                      ((A, A, X, Y, 2, 8, 0.1, S, A, -2), EINVAL), ((A, A, X, Y, 0, 8, 0.1, S, None, 0), OK)):
        add(code, "uniir_dropout_f32", *bad)
    for bad, code in (((None, A, X, Y, 2, 8, 0.1, S, I), EINVAL), ((A, A, None, None, 2, 8, 0.1, S, I), EINVAL), ((A, A, X, Y, 2, 8, 0.1, S, None), EINVAL),
                      ((A, A, X, Y, -1, 8, 0.1, S, I), EINVAL), ((A, A, X, Y, 2, 0, 0.1, S, I), EINVAL), ((A, A, X, Y, 2, 6, 0.1, S, I), EINVAL),
                      ((A, A, X, Y, 2, 8, -0.1, S, I), EINVAL), ((A, A, X, Y, 2, 8, 1.0, S, I), EINVAL), ((A, A, X, Y, 0, 8, 0.1, S, I), OK)):
        add(code, "uniir_dropout_f32_rows", *bad)
    for bad, code in (((None, Y, 2, 8, 8, 0.1, S, None, 0), EINVAL), ((H, None, 2, 8, 8, 0.1, S, None, 0), EINVAL),
                      ((H, Y, -1, 8, 8, 0.1, S, None, 0), EINVAL), ((H, Y, 2, 0, 8, 0.1, S, None, 0), EINVAL), ((H, Y, 2, 6, 8, 0.1, S, None, 0), EINVAL),
                      ((H, Y, 2, 8, 10, 0.1, S, None, 0), EINVAL), ((H, Y, 2, 8, 8, -0.1, S, None, 0), EINVAL), ((H, Y, 2, 8, 8, 1.0, S, None, 0), EINVAL),
                      ((H, Y, 2, 8, 8, 0.1, S, A, 0), EINVAL), ((H, Y, 0, 8, 8, 0.1, S, None, 0), OK)):
        add(code, "uniir_dropout_bf16", *bad)
    for bad, code in (((None, Y, 2, 8, 8, 0.1, S, I), EINVAL), ((H, None, 2, 8, 8, 0.1, S, I), EINVAL), ((H, Y, 2, 8, 8, 0.1, S, None), EINVAL),
                      ((H, Y, -1, 8, 8, 0.1, S, I), EINVAL), ((H, Y, 2, 0, 8, 0.1, S, I), EINVAL), ((H, Y, 2, 6, 8, 0.1, S, I), EINVAL),
                      ((H, Y, 2, 8, 10, 0.1, S, I), EINVAL), ((H, Y, 2, 8, 8, -0.1, S, I), EINVAL), ((H, Y, 2, 8, 8, 1.0, S, I), EINVAL),
                      ((H, Y, 0, 8, 8, 0.1, S, I), OK)):
        add(code, "uniir_dropout_bf16_rows", *bad)
    for bad, code in (((None, 8, 0.1, S), EINVAL), ((X, -1, 0.1, S), EINVAL), ((X, 8, -0.1, S), EINVAL), ((X, 8, 1.0, S), EINVAL), ((X, 0, 0.1, S), OK)):
        add(code, "uniir_dropout_mask", *bad)
    offh = C.c_void_p(b16.view.data_ptr() + 2)
    for bad, code in (((None, 2, 8, X), EINVAL), ((H, 2, 8, None), EINVAL), ((H, -1, 8, X), EINVAL), ((H, 2, 0, X), EINVAL), ((H, 0, 8, X), OK),
                      ((H, 2, 12, X), ESHAPE), ((offh, 2, 8, X), EALIGN)):
        add(code, "uniir_pool_inv_norms", *bad)
    torch.cuda.synchronize()
    f0 = _stats()
    for code, name, args in plan:
        got = getattr(lib, name)(*args, st)
        assert got == code, (name, [a if not isinstance(a, C.c_void_p) else "ptr" for a in args], got, code)
    torch.cuda.synchronize()
    for b, was in zip(outs, before):
        b.assert_all_untouched(was, "a refused or empty call")
    assert _stats() == f0, "a refused or empty call reached a reduction"
    assert len(plan) > 150
