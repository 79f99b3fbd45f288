"""uniir_attn_rel_fwd_f16 and uniir_attn_rel_fwd_long_f16 -- T5-style self-attention (scale 1, bucketed relative bias) on fp16 tensors,
forward only -- and uniir_rmsnorm_fwd_f16, on the device.

Every case of tests/attn_rel_f16_cases.py element by element against the fp64 reference and the derived bound of
tests/attention_ref.py with torch.float16 (fp16's unit roundoff and the ETA_P term for the unnormalised P); no element is left out.
Calls go through the ctypes handle with the test's own buffers (Run / Buf of tests/test_attention_paths_gpu.py): a guard band behind
every tensor and a NaN pattern outside the logical extent that must come back bit for bit.  Beyond the bound: two calls on the same
operands give the same bits; up to 512 tokens both entry points run on the same operands, both inside the bound, and the test prints
whether their bits agree (two kernels: equality is not required); refused calls return the code of the bf16 twin and write nothing.
Each case prints an OBS line with the largest |got - ref| / bound.

uniir_rmsnorm_fwd_f16: y_f32 has the bits of uniir_rmsnorm_fwd's, y_f16 is that value rounded once to fp16; each output alone; a
canary row behind y_f16 stays untouched (the pattern of tests/test_glue_f16_gpu.py)."""
import ctypes as C
import faulthandler

import pytest
import torch

import attention_ref as R
from attn_rel_f16_cases import CASES, LONG_FN, NAMES, RES_FN, RESIDENT, entry
from test_attention_paths_gpu import DEV, ERR, TAIL, Buf, Run, _fmt, _judge, _lib, _stream, _untouched

pytestmark = pytest.mark.gpu
CASE_SECONDS = 120    # a case takes a few seconds; a hung kernel ends the run here instead of at the runner's limit
F16 = torch.float16
TWIN = {RES_FN: ("uniir_attention_rel_fwd", 512), LONG_FN: ("uniir_attention_rel_fwd_long", 1024)}


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _vp(t):
    return C.c_void_p(t.data_ptr())


class RunRel16(Run):
    """the buffers of Run (api "rel": one packed fp16 qkv buffer), the call of one of the two fp16 entry points"""

    def forward(self, fn=None):
        c, W = self.c, self.W
        fn = fn or entry(c)
        self.out = Buf(self.nq, W, self.out_ld, F16)
        self.lse = Buf(1, c.batch * c.heads * c.tq, c.batch * c.heads * c.tq + TAIL, torch.float32)
        before = {"out": self.out.bits().clone(), "lse": self.lse.bits().clone()}
        it = self.items[0]
        self.emb, self.bucket = it.rel_emb.contiguous(), it.rel_bucket.contiguous()
        rc = getattr(_lib(), fn)(self.X.ptr(0), self.out.ptr(), self.lse.ptr(), _vp(self.emb), _vp(self.bucket), c.nbuckets, 1.0, c.batch,
                                 c.tq, c.heads, _stream())
        torch.cuda.synchronize()
        assert rc == 0, (c.name, fn, rc)
        _untouched(f"{c.name} out", self.out, before["out"])
        _untouched(f"{c.name} lse", self.lse, before["lse"])
        return self.item_outputs_fwd()


def _judged_twice(c, run, fref, fn):
    ratios = {}
    _judge(c, fn, run.forward(fn), fref, ratios)
    bits = run.out.bits().clone(), run.lse.bits().clone()
    run.forward(fn)
    assert torch.equal(run.out.bits(), bits[0]) and torch.equal(run.lse.bits(), bits[1]), f"{c.name}: two calls of {fn} differ"
    print(f"\nOBS {c.name} [{fn}] forward {_fmt(ratios)}")
    return bits


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_rel_fp16_forward(case):
    c = case
    assert c.dtype == F16
    items = R.build_items(c, DEV)
    fref = [it.fwd_ref()[0] for it in items]          # computed once, shared by both entry points
    run = RunRel16(c, items)
    own = _judged_twice(c, run, fref, entry(c))
    if c in RESIDENT:          # the streaming entry point takes every size: the same operands, its own kernel
        other = _judged_twice(c, run, fref, LONG_FN)
        print(f"OBS {c.name} bits of {RES_FN} and {LONG_FN} agree: out={torch.equal(own[0], other[0])} lse={torch.equal(own[1], other[1])}")


def _refusal_rows(limit):
    """(what, changes): one row each for a NULL operand, seq 0, seq above the limit, nbuckets 0 and 65, a misaligned qkv, batch 0.
    The resident entry point tests no alignment (like uniir_attention_rel_fwd), so its misaligned row also carries a size that no
    resident kernel takes: no row reaches a launch"""
    mis = {"qkv": "+2"} if limit > 512 else {"qkv": "+2", "seq": limit + 1}
    return [("qkv NULL", {"qkv": None}), ("out NULL", {"out": None}), ("lse NULL", {"lse": None}), ("rel_emb NULL", {"rel_emb": None}),
            ("rel_bucket NULL", {"rel_bucket": None}), ("seq 0", {"seq": 0}), (f"seq {limit + 1}", {"seq": limit + 1}),
            ("nbuckets 0", {"nbuckets": 0}), ("nbuckets 65", {"nbuckets": 65}), ("qkv misaligned", mis), ("batch 0", {"batch": 0})]


@pytest.mark.parametrize("fn", [RES_FN, LONG_FN])
def test_refusals_follow_the_bf16_twin_and_write_nothing(fn):
    lib = _lib()
    twin, limit = TWIN[fn]
    H, W, seq = 2, 128, 16
    X = Buf(2 * seq + 1, 3 * W, 3 * W, F16)
    X.view.normal_()
    out, lse = Buf(2 * seq + 1, W, W, F16), Buf(1, 2 * H * seq, 2 * H * seq + TAIL, torch.float32)
    emb = torch.randn(32, H, device=DEV)
    bucket = R.default_buckets(seq, seq, 32, DEV).contiguous()
    want = {"qkv NULL": "EINVAL", "out NULL": "EINVAL", "lse NULL": "EINVAL", "rel_emb NULL": "EINVAL", "rel_bucket NULL": "EINVAL",
            "seq 0": "ESHAPE", f"seq {limit + 1}": "ESHAPE", "nbuckets 0": "EINVAL", "nbuckets 65": "EINVAL",
            "qkv misaligned": "EALIGN" if limit > 512 else "ESHAPE"}
    wrong = []
    for what, change in _refusal_rows(limit):
        a = dict(qkv=X.flat.data_ptr(), out=out.flat.data_ptr(), lse=lse.flat.data_ptr(), rel_emb=emb.data_ptr(), rel_bucket=bucket.data_ptr(),
                 nbuckets=32, scale=1.0, batch=2, seq=seq, heads=H)
        for k, v in change.items():
            a[k] = a[k] + int(v) if isinstance(v, str) else v
        vals = [a[k] for k in ("qkv", "out", "lse", "rel_emb", "rel_bucket", "nbuckets", "scale", "batch", "seq", "heads")]
        before = out.bits().clone(), lse.bits().clone()
        rc = getattr(lib, fn)(*vals, _stream())
        rc_twin = getattr(lib, twin)(*vals, 0.0, 1, _stream())
        torch.cuda.synchronize()
        assert torch.equal(out.bits(), before[0]) and torch.equal(lse.bits(), before[1]), f"{fn} {what}: a refused call wrote"
        code = ERR[want[what]] if what in want else 0
        if rc != rc_twin or rc != code:
            wrong.append((what, rc, rc_twin, code))
    assert not wrong, wrong


# ------------------------------------------------------------------------------------------------------------------------- RMS norm
@pytest.mark.parametrize("rows,width,stride", [(5, 128, 128), (9, 768, 800)], ids=["5x128", "9x768-stride-800"])
def test_rmsnorm_fwd_f16_rounds_the_fp32_result_of_the_bf16_entry_point(rows, width, stride):
    from uniir_amd import ops
    g = torch.Generator().manual_seed(rows * 10007 + width)
    xs = (torch.randn(rows, stride, generator=g) * 3 + 0.5).to(DEV)
    xs[0, : width // 2] *= 1e3          # a row whose mean square is dominated by a few large elements
    xs[:, width:] = float("nan")        # behind the row: never read
    gamma = torch.randn(width, generator=g).to(DEV)
    canary = 0x7B7B
    y16 = torch.full((rows + 1, width), canary, dtype=torch.int16, device=DEV).view(F16)
    y32 = torch.empty(rows, width, device=DEV)
    ops.call("uniir_rmsnorm_fwd_f16", xs, stride, gamma, y16, y32, rows, width, 1e-6)
    b16, b32 = torch.empty(rows, width, device=DEV, dtype=torch.bfloat16), torch.empty(rows, width, device=DEV)
    ops.call("uniir_rmsnorm_fwd", xs, stride, gamma, b16, b32, rows, width, 1e-6)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(y32).all())
    assert torch.equal(y32, b32), "y_f32 of the fp16 entry point against uniir_rmsnorm_fwd's"
    assert torch.equal(y16[:rows].view(torch.int16), y32.half().view(torch.int16)), "y_f16 against y_f32 rounded once to fp16"
    assert bool((y16[rows].view(torch.int16) == canary).all())          # nothing behind the last row
    ref = (xs[:, :width].double() * torch.rsqrt(xs[:, :width].double().pow(2).mean(-1, keepdim=True) + 1e-6) * gamma.double())
    assert float((y32.double() - ref).abs().max() / ref.abs().max()) < 1e-5          # and it is the RMS norm
    only16 = torch.empty(rows, width, device=DEV, dtype=F16)          # each output alone
    ops.call("uniir_rmsnorm_fwd_f16", xs, stride, gamma, only16, None, rows, width, 1e-6)
    only32 = torch.empty(rows, width, device=DEV)
    ops.call("uniir_rmsnorm_fwd_f16", xs, stride, gamma, None, only32, rows, width, 1e-6)
    assert torch.equal(only16.view(torch.int16), y16[:rows].view(torch.int16)) and torch.equal(only32, b32)
    # the wrapper: an fp16 tensor in the 16-bit slot takes this entry point, dtype16 allocates one; bf16 as before
    kw = dict(rows=rows, width=width, x_stride=stride)
    assert torch.equal(ops.rmsnorm_fwd(xs, gamma, 1e-6, out_bf16=torch.empty_like(only16), **kw), only16)
    assert torch.equal(ops.rmsnorm_fwd(xs, gamma, 1e-6, dtype16=F16, **kw), only16)
    assert torch.equal(ops.rmsnorm_fwd(xs, gamma, 1e-6, out_f32=torch.empty_like(only32), dtype16=F16, **kw), b32)
    assert torch.equal(ops.rmsnorm_fwd(xs, gamma, 1e-6, **kw), b16)
