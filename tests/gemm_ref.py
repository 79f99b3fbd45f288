"""fp64 reference of uniir_gemm (include/uniir_hip.h) and an element-wise error bound derived from its arithmetic.

Not a test module: tests/test_gemm_paths_gpu.py compares every kernel path against it and tests/test_gemm_ref.py checks on the
CPU that it rejects corrupted results.  Inputs are the logical operands op(A) [M][K] and op(B) [K][N], already rounded to the
kernel's 16-bit type; everything else is computed in float64.

Bound of an output element with reference value r (fp64) and magnitude term T (the same sum with every term replaced by its
absolute value):
    |got - r| <= u_out * |r| + (1 + u_out) * 2 * (K + 4) * 2^-24 * T
u_out is the unit roundoff of the stored type (2^-8 bf16, 2^-11 fp16, 0 fp32); a 16-bit output also gets an absolute
eta_out, half its smallest subnormal (2^-25 for fp16), for results that round into the subnormal range.  The products of two
16-bit values are exact in fp32, so fp32 accumulation of K products in any order -- split-K slabs and their reduction, atomics, a head and a tail -- is
within (K - 1) * 2^-24 * T; the factor 2 and the + 4 cover the few fp32 operations of the epilogue (alpha, bias, row scale,
residual, the starting value of an accumulating output).  The activations run on fast fp32 approximations (hardware exp and
reciprocal, the Abramowitz-Stegun erfc): their error is bounded by ACT_EPS * |x| for act(x) and ACT_EPS for act'(x), a margin of
about 16x over the approximations' own error.  Column and row sums add the bounds of their terms plus the fp32 error of the sum.
"""
import math

import torch

EPS32 = 2.0 ** -24
ACT_EPS = 2.0 ** -16
ACT_LIPSCHITZ = 1.13          # max |act'| over the three activations (GELU 1.129, QuickGELU 1.10, ReLU 1)
U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
ETA_OUT = {torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25, torch.float32: 0.0}     # half the smallest subnormal

EPI_BF16, EPI_BIAS_ACT, EPI_RESID_F32, EPI_DACT, EPI_F32, EPI_ATOMIC_F32, EPI_ACT_ONLY = range(7)
ACT_QUICKGELU, ACT_GELU_ERF, ACT_RELU = range(3)


def round16(x, dtype):
    """x rounded to the 16-bit type, as float64"""
    return x.to(dtype).double()


def act_fwd(x, act):
    x = x.double()
    if act == ACT_QUICKGELU:
        return x * torch.sigmoid(1.702 * x)
    if act == ACT_GELU_ERF:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return x.clamp_min(0.0)


def act_bwd(x, act):
    x = x.double()
    if act == ACT_QUICKGELU:
        s = torch.sigmoid(1.702 * x)
        return s * (1.0 + 1.702 * x * (1.0 - s))
    if act == ACT_GELU_ERF:
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    return (x > 0).double()


def _col(v):
    return None if v is None else v.double()


def gemm_reference(opA, opB, *, epilogue, alpha=1.0, bias=None, resid=None, row_scale=None, aux=None, act=ACT_QUICKGELU,
                   c0=None, out16=torch.bfloat16, got_f=None, got_c=None, colsum0=None, colsum_rounded=False, rowsum0=None):
    """-> dict name -> (reference, bound), float64, for the outputs the descriptor produces: "C", "C2" (BIAS_ACT: act of the
    kernel's own f = got_f; RESID_F32: bf16 copy of the kernel's own C = got_c; DACT: act(aux)), "colsum" when colsum0 is given
    (its starting value; colsum_rounded: summed from the rounded 16-bit result, the separate pass), "rowsum" when rowsum0 is
    given.  bias [N], resid / c0 [M][N], row_scale [M], aux [M][N] (bf16 values) are the logical operands."""
    A, B = opA.double(), opB.double()
    K = A.shape[1]
    v = alpha * (A @ B)
    T = abs(alpha) * (A.abs() @ B.abs())
    bias, resid, row_scale, aux, c0 = _col(bias), _col(resid), _col(row_scale), _col(aux), _col(c0)
    if bias is not None:
        v = v + bias
        T = T + bias.abs()
    acc = lambda t: 2.0 * (K + 4) * EPS32 * t          # noqa: E731  fp32 accumulation + epilogue arithmetic
    out = {}
    pre = None          # value the column sums add (before rounding) and its bound without the output rounding
    if epilogue in (EPI_BF16, EPI_BIAS_ACT):
        u = U_OUT[out16]
        e = acc(T)
        eta = ETA_OUT[out16]
        out["C"] = (v, u * v.abs() + (1 + u) * e + eta)
        pre = (v, e)
        if epilogue == EPI_BIAS_ACT:
            f = got_f.double()
            g = act_fwd(f, act)
            out["C2"] = (g, u * g.abs() + (1 + u) * ACT_EPS * f.abs() + eta)
    elif epilogue == EPI_ACT_ONLY:
        u = U_OUT[out16]
        bf = u * v.abs() + (1 + u) * acc(T)             # the kernel's f = 16-bit(v + bias), up to eta
        g = act_fwd(v, act)
        eta = ETA_OUT[out16]
        out["C"] = (g, u * g.abs() + (1 + u) * (ACT_LIPSCHITZ * (bf + eta) + ACT_EPS * (v.abs() + bf)) + eta)
    elif epilogue == EPI_RESID_F32:
        if row_scale is not None:
            v = v * row_scale[:, None]
            T = T * row_scale.abs()[:, None]
        if resid is not None:
            v = v + resid
            T = T + resid.abs()
        e = acc(T)
        out["C"] = (v, e)
        pre = (v, e)
        if got_c is not None:
            gc = got_c.double()
            out["C2"] = (gc, U_OUT[torch.bfloat16] * gc.abs() + ETA_OUT[torch.bfloat16])
    elif epilogue == EPI_DACT:
        d = act_bwd(aux, act)
        r = v * d
        e = acc(T * d.abs()) + ACT_EPS * v.abs()
        out["C"] = (r, U_OUT[torch.bfloat16] * r.abs() + (1 + U_OUT[torch.bfloat16]) * e + ETA_OUT[torch.bfloat16])
        pre = (r, e)
        g = act_fwd(aux, act)
        out["C2"] = (g, U_OUT[torch.bfloat16] * g.abs() + (1 + U_OUT[torch.bfloat16]) * ACT_EPS * aux.abs() + ETA_OUT[torch.bfloat16])
    elif epilogue == EPI_F32:
        e = acc(T)
        out["C"] = (v, e)
        pre = (v, e)
    elif epilogue == EPI_ATOMIC_F32:
        if c0 is not None:
            v = v + c0
            T = T + c0.abs()
        out["C"] = (v, acc(T))
    else:
        raise ValueError(epilogue)
    if colsum0 is not None:
        r, e = pre
        M = r.shape[0]
        cs0 = colsum0.double()
        bound = e.sum(0) + 2.0 * (M + 2) * EPS32 * (r.abs().sum(0) + cs0.abs())
        if colsum_rounded:
            u = U_OUT[out16] if epilogue != EPI_DACT else U_OUT[torch.bfloat16]
            dt16 = out16 if epilogue != EPI_DACT else torch.bfloat16
            bound = bound + u * r.abs().sum(0) + u * e.sum(0) + M * ETA_OUT[dt16]
        out["colsum"] = (cs0 + r.sum(0), bound)
    if rowsum0 is not None:
        rs0 = rowsum0.double()
        out["rowsum"] = (rs0 + A.sum(1), 2.0 * (K + 2) * EPS32 * (A.abs().sum(1) + rs0.abs()))
    return out


def violations(got, ref, bound):
    """bool mask of the elements outside the bound (NaN / Inf count as outside)"""
    d = (got.double() - ref).abs()
    return ~(d <= bound)


def check(got, ref, bound, what=""):
    bad = violations(got, ref, bound)
    if bool(bad.any()):
        idx = torch.nonzero(bad)
        first = tuple(int(i) for i in idx[0])
        d = (got.double() - ref).abs()
        worst = torch.argmax(torch.where(bad, d / bound.clamp_min(1e-300), torch.zeros_like(d)).flatten())
        wi = tuple(int(i) for i in torch.unravel_index(worst, d.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements outside the bound; first at {first} "
                             f"(got {float(got[first])}, ref {float(ref[first])}, bound {float(bound[first]):.3g}); "
                             f"worst at {wi} (got {float(got[wi])}, ref {float(ref[wi])}, bound {float(bound[wi]):.3g})")
