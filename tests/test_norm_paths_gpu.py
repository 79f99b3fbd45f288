"""uniir_layernorm_* / uniir_rmsnorm_* on every kernel instance against the fp64 reference of tests/fp32_ref.py, element by element.

The case tables are tests/fp32_cases.py's NORM_FWD / NORM_BWD (tests/test_fp32_ref.py asserts on the CPU that every case reaches the
instance it names).  Paths in csrc/norm.hip:
  NC2p NC2e NC3p NC3e NC4p NC4e NC8p NC8e   ln_fwd_kernel<NC, EXACT> / ln_bwd_kernel<NC, DY_F32, EXACT>: NC float4 chunks per lane,
                                            e = width == 256 NC (no predication), p = predicated chunks
Forward: every width on both sides of each NC, rows 1 / 3 / 4 / 5 / 37, the three output combinations, x_stride = width and
3 width + 8, and 8231 rows (more than any resident grid holds, so the persistent row loop strides).  Backward: the sixteen instances
(NC x EXACT x dy type), each once with every option on (dres read with dx_stride > width, dx_bf16, dx_colsum, branch_scale holding
0, 1 and 1 / 0.7 through uniir_layernorm_bwd_ex) and once with every option off -- the options are run-time arguments of one
instance, so the two cases pair every instance with both values of every option; five more cases switch the options one by one
(dres without dx_bf16, dx_stride > width without dres, dx_colsum without branch_scale, ...); uniir_rmsnorm_bwd runs the same
instances with both dy types.  The 8231-row cases feed integer dy, so dbeta is exact and loses no row in the strided loop.  Reduction forms: one workgroup (rows <= 4: direct adds, uniir_reduce_stats does not move), stored partials with the
stream's scratch (run twice, bitwise equal, no fallback counted), and atomics with the scratch removed or one byte too small (one
fallback counted per launch).  dgamma, dbeta and dx_colsum always start from non-zero contents: the result is prior + sum.

Every tensor sits in a buffer with guard rows behind it and, where it has a stride, a NaN pattern between width and the stride; after
the call everything outside the logical extent holds the pattern bit for bit (the columns between width and dx_stride included), and
no input padding reaches a result (NaN is a violation).  The fp16 16-bit output is reachable only through the tower entry point
(uniir_clip_tower.dtype16) and is not covered here."""
import ctypes as C

import pytest
import torch

import fp32_cases as T
import fp32_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
ERR = {"EINVAL": -1, "ESHAPE": -2}
TAIL = 64


def _lib():
    from uniir_amd import _lib
    return _lib.load()


def _p(b):
    if b is None:
        return None
    return C.c_void_p(b.view.data_ptr() if isinstance(b, T.Buf) else b.data_ptr())


def _stats():
    f, m = C.c_int64(), C.c_int64()
    assert _lib().uniir_reduce_stats(C.byref(f), C.byref(m), 0) == 0
    return f.value, m.value


class _Scratch:
    """the stream's reduction scratch for one call: ops' buffer ("on"), none ("off") or a temporary one of `bytes`"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from uniir_amd import ops
        self.lib = _lib()
        self.stream = ops._stream()            # registers ops' buffer for the current stream
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


def _vec(t):
    """[n] fp32 with TAIL spare floats of NaN pattern behind it"""
    return T.Buf(1, t.numel(), t.numel() + TAIL, device=DEV).set(t[None, :])


def _obs(name, ratios):
    print(f"\nOBS {name} worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


def _check_all(c, got, ref):
    ratios = {}
    for k, g in got.items():
        R.check(g, *ref[k], f"{c.name} ({c.path}) {k}")
        ratios[k] = R.worst_ratio(g, *ref[k])
    _obs(f"{c.name} {c.path}", ratios)


# ------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("c", T.NORM_FWD, ids=[c.name for c in T.NORM_FWD])
def test_norm_fwd_path(c):
    d = T.norm_inputs(c, DEV)
    x = T.Buf(c.rows, c.width, c.x_stride, device=DEV).set(d["x"])
    gamma, beta = _vec(d["gamma"]), _vec(d["beta"])
    y16 = T.Buf(c.rows, c.width, dtype=BF16, device=DEV) if c.outs in ("bf16", "both") else None
    y32 = T.Buf(c.rows, c.width, device=DEV) if c.outs in ("f32", "both") else None
    outs = {k: b for k, b in (("y_bf16", y16), ("y_f32", y32)) if b is not None}
    before = {k: b.bits().clone() for k, b in outs.items()}
    from uniir_amd import ops
    lib, st = _lib(), ops._stream()
    if c.rms:
        rc = lib.uniir_rmsnorm_fwd(_p(x), c.x_stride, _p(gamma), _p(y16), _p(y32), c.rows, c.width, c.eps, st)
    else:
        rc = lib.uniir_layernorm_fwd(_p(x), c.x_stride, _p(gamma), _p(beta), _p(y16), _p(y32), c.rows, c.width, c.eps, st)
    torch.cuda.synchronize()
    assert rc == 0, (c.name, rc)
    for k, b in outs.items():
        b.assert_outside_untouched(before[k], f"{c.name} {k}")
    ref = R.norm_fwd(x.view, gamma.view[0], beta.view[0], c.eps, c.rms)
    _check_all(c, {k: b.view for k, b in outs.items()}, ref)
    if c.data == "const" and y32 is not None:          # variance 0: y is beta, to within the bound
        R.check(y32.view[0], beta.view[0].double(), ref["y_f32"][1][0], f"{c.name} constant row")


# ------------------------------------------------------------------------------------------------------------------ backward
class _Bwd:
    def __init__(self, c, d):
        self.c = c
        R_, W = c.rows, c.width
        self.x = T.Buf(R_, W, c.x_stride, device=DEV).set(d["x"])
        self.gamma = _vec(d["gamma"])
        self.dy = T.Buf(R_, W, dtype=torch.float32 if c.dy_f32 else BF16, device=DEV).set(d["dy"])
        self.dres = T.Buf(R_, W, c.dx_stride, device=DEV).set(d["dres"]) if "dres" in d else None
        self.dx = T.Buf(R_, W, c.dx_stride, device=DEV)
        self.dxb = T.Buf(R_, W, dtype=BF16, device=DEV) if c.has("b") else None
        self.dgamma = _vec(d["dgamma0"])
        self.dbeta = _vec(d["dbeta0"]) if not c.rms else None
        self.colsum = _vec(d["colsum0"]) if "colsum0" in d else None
        self.bscale = _vec(d["branch_scale"]) if "branch_scale" in d else None
        self.outs = {k: b for k, b in (("dx_f32", self.dx), ("dx_bf16", self.dxb), ("dgamma", self.dgamma), ("dbeta", self.dbeta),
                                        ("dx_colsum", self.colsum)) if b is not None}
        self.before = {k: b.bits().clone() for k, b in self.outs.items()}

    def call(self, scratch):
        c, lib = self.c, _lib()
        a = (_p(self.x), c.x_stride, _p(self.gamma), _p(self.dy), int(c.dy_f32), _p(self.dres), _p(self.dx), c.dx_stride, _p(self.dxb),
             _p(self.dgamma))
        with _Scratch(scratch) as st:
            if c.rms:
                rc = lib.uniir_rmsnorm_bwd(*a, c.rows, c.width, c.eps, st)
            elif self.bscale is not None:
                rc = lib.uniir_layernorm_bwd_ex(*a, _p(self.dbeta), _p(self.colsum), _p(self.bscale), c.rows, c.width, c.eps, st)
            else:
                rc = lib.uniir_layernorm_bwd(*a, _p(self.dbeta), _p(self.colsum), c.rows, c.width, c.eps, st)
        assert rc == 0, (c.name, rc)

    def got(self):
        return {k: (b.view[0] if k in ("dgamma", "dbeta", "dx_colsum") else b.view) for k, b in self.outs.items()}


@pytest.mark.parametrize("c", T.NORM_BWD, ids=[c.name for c in T.NORM_BWD])
def test_norm_bwd_path(c):
    d = T.norm_inputs(c, DEV)
    run = _Bwd(c, d)
    wg = min(c.workgroups, 4 * 256) if c.rows <= 4096 else None          # the long cases are clipped to the resident grid
    need = None if wg is None else wg * 3 * c.width * 4
    scratch = c.scratch if c.scratch != "short" else need - 1
    from uniir_amd import ops
    ops._stream()                                # the stream's buffer is registered before the counters are read
    f0, m0 = _stats()
    run.call(scratch)
    f1, m1 = _stats()
    for k, b in run.outs.items():
        b.assert_outside_untouched(run.before[k], f"{c.name} {k}")
    ref = R.norm_bwd(run.x.view, run.gamma.view[0], run.dy.view, c.eps, c.rms, dres=d.get("dres"),
                     branch_scale=d.get("branch_scale"), dgamma0=d["dgamma0"], dbeta0=d["dbeta0"], colsum0=d.get("colsum0"))
    if "dx_bf16" not in run.outs:
        ref.pop("dx_bf16")
    assert set(ref) == set(run.outs)
    _check_all(c, run.got(), ref)
    assert bool(torch.isfinite(run.dx.view).all())
    if c.workgroups == 1:                        # direct adds of one workgroup: no scratch asked for, nothing counted
        assert (f1, m1) == (f0, m0), (c.name, (f0, m0), (f1, m1))
    elif c.scratch == "on":
        assert f1 == f0, f"{c.name}: {f1 - f0} fallbacks with the stream's scratch registered"
        again = _Bwd(c, d)
        again.call("on")
        for k, b in again.outs.items():
            assert torch.equal(b.bits(), run.outs[k].bits()), f"{c.name}: {k} differs between two runs"
        assert _stats()[0] == f0
    else:
        assert f1 == f0 + 1, f"{c.name}: fallbacks moved by {f1 - f0}, one launch without enough scratch"
        assert m1 >= need


# -------------------------------------------------------------------------------------------------------------------- errors
def test_norm_argument_errors():
    from uniir_amd import ops
    lib, st = _lib(), ops._stream()
    W, rows = 512, 5
    x = T.Buf(rows, 2056, device=DEV).set(torch.randn(rows, 2056, device=DEV))
    g = _vec(torch.randn(2056, device=DEV))
    y32, y16 = T.Buf(rows, 2056, device=DEV), T.Buf(rows, 2056, dtype=BF16, device=DEV)
    dy = T.Buf(rows, 2056, device=DEV).set(torch.randn(rows, 2056, device=DEV))
    dx, dg, db = T.Buf(rows, 2056, device=DEV), _vec(torch.ones(2056, device=DEV)), _vec(torch.ones(2056, device=DEV))
    outs = (y32, y16, dx, dg, db)
    before = [b.bits().clone() for b in outs]

    def fwd(width=W, xs=W, r=rows, xp=x, gp=g, bp=g, y=y32, rms=False):
        if rms:
            return lib.uniir_rmsnorm_fwd(_p(xp), xs, _p(gp), _p(y16), _p(y), r, width, 1e-6, st)
        return lib.uniir_layernorm_fwd(_p(xp), xs, _p(gp), _p(bp), _p(y16), _p(y), r, width, 1e-5, st)

    def bwd(width=W, xs=W, dxs=W, r=rows, xp=x, dyp=dy, dxp=dx, dgp=dg, dbp=db, rms=False):
        a = (_p(xp), xs, _p(g), _p(dyp), 1, None, _p(dxp), dxs, None, _p(dgp))
        if rms:
            return lib.uniir_rmsnorm_bwd(*a, r, width, 1e-6, st)
        return lib.uniir_layernorm_bwd(*a, _p(dbp), None, r, width, 1e-5, st)

    for rms in (False, True):
        for kw in ({"width": 510}, {"width": 2052, "xs": 2052}, {"xs": 514}):
            assert fwd(rms=rms, **kw) == ERR["ESHAPE"], (rms, kw)
            assert bwd(rms=rms, **kw) == ERR["ESHAPE"], (rms, kw)
        assert bwd(rms=rms, dxs=514) == ERR["ESHAPE"]
        assert fwd(rms=rms, xp=None) == ERR["EINVAL"] and fwd(rms=rms, gp=None) == ERR["EINVAL"]
        assert bwd(rms=rms, xp=None) == ERR["EINVAL"] and bwd(rms=rms, dyp=None) == ERR["EINVAL"]
        assert bwd(rms=rms, dxp=None) == ERR["EINVAL"] and bwd(rms=rms, dgp=None) == ERR["EINVAL"]
        assert fwd(rms=rms, r=0) == 0 and bwd(rms=rms, r=0) == 0
    assert fwd(bp=None) == ERR["EINVAL"] and bwd(dbp=None) == ERR["EINVAL"]
    none16 = lib.uniir_layernorm_fwd(_p(x), W, _p(g), _p(g), None, None, rows, W, 1e-5, st)
    assert none16 == ERR["EINVAL"]
    torch.cuda.synchronize()
    for b, was in zip(outs, before):
        b.assert_all_untouched(was, "a refused or empty call")
