"""The gradient guard's kernels through the C ABI against tests/grad_guard_ref.py: uniir_grad_guard on every count at which the code
takes another path (empty, below one 16-byte group, a live count % 4 tail, a partial chunk, exactly one chunk, one element into the
next, two chunks and a tail), three value sets, two scales, one range and three; the non-finite scan; the fp32 overflow of the norm;
same input, same bits on two streams; uniir_adamw_step_guarded against uniir_adamw_step and tests/fp32_ref.py; the refusals.

Bound: |sumsq_dev - sumsq_ref| <= n * 2^-53 * sumsq_ref (grad_guard_ref.bound: every term is exact and non-negative).  norm and coef
are compared for EQUALITY with the fp32 formulas applied to the bits the device wrote."""
import ctypes as C

import numpy as np
import pytest
import torch

import fp32_cases as T
import fp32_ref as R
import grad_guard_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda"
EINVAL, EALIGN = -1, -3
PATTERN = 0x5A5A5A5A5A5A5A5A


def _lib():
    from uniir_amd import _lib
    return _lib.load()


def _st():
    from uniir_amd import ops
    return ops._stream()


def _chunk():
    return int(_lib().uniir_grad_guard_chunk())


def _read(ctl):
    from uniir_amd import _lib
    torch.cuda.synchronize()
    return _lib.GradCtl.from_buffer_copy(ctl.cpu().numpy().tobytes())


class Ranges:
    """host arrays over device ranges that start 16 bytes into a 256-byte block each: 16-byte aligned and not 256-byte aligned"""

    def __init__(self, arrays):
        offs, cur = [], 4
        for a in arrays:
            offs.append(cur)
            cur += (a.size + 3) // 4 * 4 + 4
            if (4 * cur) % 256 == 0:
                cur += 4
        self.flat = torch.zeros(cur + 64, dtype=torch.float32, device=DEV)
        assert self.flat.data_ptr() % 256 == 0
        for o, a in zip(offs, arrays):
            if a.size:
                self.flat[o:o + a.size] = torch.from_numpy(a).to(DEV)
        n = len(arrays)
        self.ptrs = (C.c_void_p * max(1, n))(*[self.flat.data_ptr() + 4 * o for o in offs])
        self.counts = (C.c_int64 * max(1, n))(*[a.size for a in arrays])
        self.n = n
        assert all(p % 16 == 0 and p % 256 != 0 for p in self.ptrs[:n])
        self.ws_bytes = int(_lib().uniir_grad_guard_workspace_bytes(self.counts, n))
        self.ws = torch.full((max(256, self.ws_bytes),), 0xA5, dtype=torch.uint8, device=DEV)
        self.ctl = torch.zeros(8, dtype=torch.int64, device=DEV)

    def run(self, scale, max_norm=0.0, skip=0):
        rc = _lib().uniir_grad_guard(self.ptrs, self.counts, self.n, scale, max_norm, skip, self.ctl.data_ptr(), self.ws.data_ptr(),
                                     self.ws_bytes, _st())
        assert rc == 0
        return _read(self.ctl)


def _check(c, arrays, scale, max_norm=0.0, skip=0, what=""):
    """one device result against the reference: the sum inside the bound; everything else exact"""
    ref, n, first_bad = G.sumsq(arrays, scale)
    bound = G.bound(n, ref)
    err = abs(c.sumsq - ref)
    print(f"\nOBS grad_guard {what}: n {n} sumsq_dev {c.sumsq!r} ref {ref!r} |diff| {err:.3e} bound {bound:.3e}")
    assert err <= bound, f"{what}: |{c.sumsq!r} - {ref!r}| = {err:.3e} > {bound:.3e}"
    norm, nonfinite, sk, coef = G.decide(c.sumsq, first_bad is not None, max_norm, skip)
    assert np.float32(c.norm).tobytes() == norm.tobytes(), f"{what}: norm {c.norm!r} != fl32(sqrt(sumsq_dev)) {norm!r}"
    assert np.float32(c.coef).tobytes() == coef.tobytes(), f"{what}: coef {c.coef!r} != {coef!r}"
    assert (c.nonfinite, c.skip) == (int(nonfinite), int(sk)), what
    if first_bad is None:
        assert (c.first_bad_range, c.first_bad_chunk, c.first_bad_index) == (-1, -1, -1), what
    else:
        assert (c.first_bad_range, c.first_bad_chunk, c.first_bad_index) == (first_bad[0], first_bad[1] // _chunk(), first_bad[1]), what


@pytest.mark.parametrize("kind", G.KINDS)
def test_single_range_every_count(kind):
    for n in G.counts(_chunk()):
        g = G.values(kind, n)
        r = Ranges([g])
        for i, scale in enumerate(G.SCALES):
            # max_norm chosen against the reference so that one scale clips and one does not
            max_norm = float(np.sqrt(G.sumsq(g, scale)[0])) * (0.37 if i == 0 else 3.0)
            c = r.run(scale, max_norm=max_norm)
            _check(c, [g], scale, max_norm, what=f"{kind} n {n} scale {scale}")
            assert (c.steps_seen, c.steps_skipped) == (i + 1, 0)
            if n and i == 0:
                assert 0 < c.coef < 1
        assert bool((r.ws[r.ws_bytes:] == 0xA5).all()), "written behind the workspace"


def test_empty_inputs():
    r = Ranges([])
    c = r.run(1.0, max_norm=1.0, skip=1)
    assert (c.sumsq, c.norm, c.coef, c.nonfinite, c.skip, c.first_bad_range) == (0.0, 0.0, 1.0, 0, 0, -1)
    z = np.zeros(0, dtype=np.float32)
    r = Ranges([z, z])
    c = r.run(1.0, max_norm=1.0, skip=1)
    assert (c.sumsq, c.norm, c.coef, c.nonfinite, c.skip, c.steps_seen) == (0.0, 0.0, 1.0, 0, 0, 1)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("scale", G.SCALES)
def test_three_ranges_off_the_256_byte_grid(kind, scale):
    ch = _chunk()
    arrays = [G.values(kind, n, seed=s) for s, n in enumerate((1003, ch + 1, 5))]
    r = Ranges(arrays)
    _check(r.run(scale, max_norm=1.0), arrays, scale, 1.0, what=f"three ranges {kind} scale {scale}")
    # with an empty range in the middle the indices of the others stay
    arrays = [arrays[0], np.zeros(0, dtype=np.float32), arrays[2]]
    arrays[2] = arrays[2].copy()
    arrays[2][3] = np.inf
    c = Ranges(arrays).run(scale)
    _check(c, arrays, scale, what="empty middle range")
    assert (c.first_bad_range, c.first_bad_index) == (2, 3)


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf], ids=["nan", "inf", "-inf"])
def test_nonfinite_scan(bad):
    ch = _chunk()
    # (count, planted index): element 0, the last element of a count % 4 tail (in the first chunk and in the second), the last
    # element of a chunk, the first of the next
    for n, at in ((1003, 0), (1003, 1002), (ch + 1, ch), (2 * ch + 5, ch - 1), (2 * ch + 5, ch), (2 * ch + 5, 2 * ch + 4)):
        g = G.values("randn", n)
        g[at] = bad
        for skip in (0, 1):
            c = Ranges([g]).run(1.0, max_norm=1.0, skip=skip)
            _check(c, [g], 1.0, 1.0, skip, what=f"{bad} at {at} of {n}, skip {skip}")
            assert c.nonfinite == 1 and (c.first_bad_range, c.first_bad_chunk) == (0, at // ch) and c.skip == skip
            assert c.coef == (0.0 if skip else 1.0) and c.steps_skipped == skip
    # in the third range, behind a second one that is clean; and two bad elements: the lowest is reported
    arrays = [G.values("randn", n, seed=s) for s, n in enumerate((1003, ch + 1, 5))]
    arrays[2][4] = bad
    c = Ranges(arrays).run(0.5, skip=1)
    _check(c, arrays, 0.5, 0.0, 1, what=f"{bad} in the third range")
    assert (c.first_bad_range, c.first_bad_chunk, c.first_bad_index, c.skip) == (2, 0, 4, 1)
    arrays[1][ch] = bad
    arrays[1][17] = bad
    c = Ranges(arrays).run(0.5)
    _check(c, arrays, 0.5, what="lowest of three")
    assert (c.first_bad_range, c.first_bad_chunk, c.first_bad_index) == (1, 0, 17)


def test_finite_gradient_whose_scaled_value_overflows_is_nonfinite():
    g = G.values("randn", 1003)
    g[500] = 3e38
    c = Ranges([g]).run(2.0)
    _check(c, [g], 2.0, what="g * scale overflows")
    assert c.nonfinite == 1 and c.first_bad_index == 500


def test_norm_overflow_in_fp32_counts_as_nonfinite():
    g = np.full(1003, 1e38, dtype=np.float32)
    for skip in (0, 1):
        c = Ranges([g]).run(1.0, max_norm=1.0, skip=skip)
        _check(c, [g], 1.0, 1.0, skip, what="1e38 x 1003")
        assert np.isfinite(c.sumsq) and np.isinf(c.norm) and c.nonfinite == 1 and c.first_bad_range == -1 and c.skip == skip


def test_same_input_same_bits_on_two_streams():
    ch = _chunk()
    arrays = [G.values("mixed", 2 * ch + 5), G.values("randn", 1003)]
    r = Ranges(arrays)
    a = r.run(0.5).sumsq
    b = r.run(0.5).sumsq
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        c = r.run(0.5).sumsq
    bits = [np.float64(x).tobytes() for x in (a, b, c)]
    assert bits[0] == bits[1] == bits[2]


# ---- guarded AdamW -------------------------------------------------------------------------------------------------------------
def _ctl(coef=1.0, skip=0):
    from uniir_amd import _lib
    c = _lib.GradCtl(sumsq=1.0, norm=1.0, coef=coef, nonfinite=skip, skip=skip, first_bad_range=-1, first_bad_chunk=-1,
                     first_bad_index=-1, steps_seen=3, steps_skipped=skip)
    return torch.frombuffer(bytearray(bytes(c)), dtype=torch.int64).to(DEV)


def _adam(name, p, g, m, v, s, count, wd, step, gs, ctl=None):
    a = T.ADAM
    args = [p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), s.data_ptr() if s is not None else None, count, a["lr"], a["b1"],
            a["b2"], a["eps"], wd, step, gs]
    if ctl is not None:
        args.append(ctl.data_ptr() if isinstance(ctl, torch.Tensor) else ctl)
    return getattr(_lib(), name)(*args, _st())


def _state(count):
    """p, g, m, v with 64 spare elements of a NaN pattern behind `count`, and a bf16 shadow"""
    out = []
    for t in T.adamw_inputs(count, DEV):
        out.append(torch.cat([t, torch.full((64,), float("nan"), device=DEV)]))
    return out + [torch.zeros(count + 64, dtype=torch.bfloat16, device=DEV)]


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


@pytest.mark.parametrize("shadow", [True, False], ids=["shadow", "no_shadow"])
@pytest.mark.parametrize("count", [5, 1003, 4096])
def test_guarded_adamw(count, shadow):
    wd, step, gs = 0.2, 3, 0.5
    base = _state(count)
    # coef = 1, skip = 0: uniir_adamw_step's bits
    plain, guarded = [t.clone() for t in base], [t.clone() for t in base]
    assert _adam("uniir_adamw_step", *plain[:4], plain[4] if shadow else None, count, wd, step, gs) == 0
    assert _adam("uniir_adamw_step_guarded", *guarded[:4], guarded[4] if shadow else None, count, wd, step, gs, _ctl(1.0, 0)) == 0
    torch.cuda.synchronize()
    for a, b, name in zip(plain, guarded, ("param", "grad", "exp_avg", "exp_avg_sq", "shadow")):
        assert torch.equal(_bits(a), _bits(b)), f"coef 1: {name} differs from uniir_adamw_step"
    assert not torch.equal(_bits(guarded[0]), _bits(base[0]))
    # skip = 1 with a NaN gradient: nothing moves
    skipped = [t.clone() for t in base]
    skipped[1][count // 2] = float("nan")
    want = [t.clone() for t in skipped]
    assert _adam("uniir_adamw_step_guarded", *skipped[:4], skipped[4] if shadow else None, count, wd, step, gs, _ctl(0.0, 1)) == 0
    torch.cuda.synchronize()
    for a, b, name in zip(want, skipped, ("param", "grad", "exp_avg", "exp_avg_sq", "shadow")):
        assert torch.equal(_bits(a), _bits(b)), f"skip: {name} moved"
    # coef = 0.37: the fp64 step of the pre-scaled gradient fl32(fl32(g * gs) * coef) at grad_scale 1
    clipped = [t.clone() for t in base]
    assert _adam("uniir_adamw_step_guarded", *clipped[:4], clipped[4] if shadow else None, count, wd, step, gs, _ctl(0.37, 0)) == 0
    torch.cuda.synchronize()
    g_pre = (base[1][:count] * np.float32(gs)) * np.float32(0.37)
    ref = R.adamw_step(base[0][:count], g_pre, base[2][:count], base[3][:count], wd=wd, step=step, grad_scale=1.0, **T.ADAM)
    worst = {}
    for k, i in (("param", 0), ("exp_avg", 2), ("exp_avg_sq", 3)):
        R.check(clipped[i][:count], *ref[k], f"guarded adamw count {count} {k}")
        worst[k] = R.worst_ratio(clipped[i][:count], *ref[k])
        assert torch.equal(_bits(clipped[i][count:]), _bits(base[i][count:])), "written behind count"
    print(f"\nOBS guarded adamw count {count} coef 0.37 worst |got - ref| / bound: " + ", ".join(f"{k} {r:.3f}" for k, r in worst.items()))
    if shadow:
        assert torch.equal(_bits(clipped[4][:count]), _bits(clipped[0][:count].to(torch.bfloat16))), "the shadow is not bf16(param)"
    else:
        assert torch.equal(_bits(clipped[4]), _bits(base[4])), "a shadow that was not passed changed"


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing():
    lib = _lib()
    g = G.values("randn", 1003)
    r = Ranges([g])
    r.ctl.fill_(PATTERN)
    ws_was = r.ws.clone()
    ctl, ws = r.ctl.data_ptr(), r.ws.data_ptr()

    def call(ptrs=r.ptrs, counts=r.counts, n=1, scale=1.0, max_norm=1.0, ctl=ctl, ws=ws, ws_bytes=r.ws_bytes):
        return lib.uniir_grad_guard(ptrs, counts, n, scale, max_norm, 1, ctl, ws, ws_bytes, _st())

    neg = (C.c_int64 * 1)(-5)
    odd = (C.c_void_p * 1)(r.ptrs[0] + 4)
    null = (C.c_void_p * 1)(None)
    assert call(ctl=None) == EINVAL and call(ptrs=null) == EINVAL and call(ws=None) == EINVAL and call(ptrs=None) == EINVAL
    assert call(counts=neg) == EINVAL and call(scale=float("nan")) == EINVAL and call(scale=-1.0) == EINVAL
    assert call(max_norm=float("nan")) == EINVAL and call(ws_bytes=r.ws_bytes - 1) == EINVAL
    assert call(ptrs=odd) == EALIGN and call(ctl=ctl + 8) == EALIGN and call(ws=ws + 16) == EALIGN
    torch.cuda.synchronize()
    assert bool((r.ctl == PATTERN).all()) and torch.equal(r.ws, ws_was)
    # the guarded step
    base = _state(1003)
    st = [t.clone() for t in base]
    good = _ctl(1.0, 0)
    assert _adam("uniir_adamw_step_guarded", *st[:4], st[4], 1003, 0.2, 1, 1.0, 0) == EINVAL               # NULL control block
    assert _adam("uniir_adamw_step_guarded", *st[:4], st[4], -1, 0.2, 1, 1.0, good) == EINVAL
    assert _adam("uniir_adamw_step_guarded", *st[:4], st[4], 1003, 0.2, 0, 1.0, good) == EINVAL
    assert _adam("uniir_adamw_step_guarded", *st[:4], st[4], 1003, 0.2, 1, 1.0, good.data_ptr() + 8) == EALIGN
    assert _adam("uniir_adamw_step_guarded", st[0][1:], *st[1:4], st[4], 1000, 0.2, 1, 1.0, good) == EALIGN
    torch.cuda.synchronize()
    for a, b in zip(base, st):
        assert torch.equal(_bits(a), _bits(b))
