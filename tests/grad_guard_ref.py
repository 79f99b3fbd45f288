"""The numpy reference of the gradient guard (include/uniir_hip.h [OPT] gradient guard), and the cases its tests share.

x = fl32(g * fl32(scale)) per element, the value AdamW consumes.  A finite x contributes the exact fp64 square of x (a 24-bit
significand squared fits 53 bits); a non-finite x contributes nothing and raises the flag.  sumsq_ref is math.fsum of those squares:
the correctly rounded exact sum.  Every term is exact and non-negative, so ANY order of n floating-point additions is within
n * 2^-53 * sumsq_ref of it: each of the n - 1 additions has relative error <= 2^-53 on a partial sum that never exceeds the total,
which gives (n - 1) * 2^-53 * sumsq to first order, and the spare 2^-53 * sumsq covers the second-order term (n * 2^-53)^2 / 2 * sumsq
for every n below 1e8; the tests stay below 2^18 -- bound().  The flags and the coefficient are restated in np.float32 arithmetic
exactly as the header writes them."""
import math

import numpy as np

F32 = np.float32
U = 2.0 ** -53


def scaled(g, scale):
    with np.errstate(over="ignore", invalid="ignore"):
        return (np.asarray(g, dtype=F32) * F32(scale)).astype(F32)


def sumsq(ranges, scale):
    """ranges: a list of fp32 arrays (or one array) -> (sumsq_ref, n, first_bad) with first_bad = (range, element) of the lowest
    non-finite x, or None"""
    if isinstance(ranges, np.ndarray):
        ranges = [ranges]
    terms, n, first_bad = [], 0, None
    for r, g in enumerate(ranges):
        x = scaled(g, scale)
        ok = np.isfinite(x)
        if first_bad is None and not ok.all():
            first_bad = (r, int(np.argmin(ok)))
        xd = x[ok].astype(np.float64)
        terms.append(xd * xd)
        n += x.size
    return math.fsum(np.concatenate(terms).tolist()) if terms else 0.0, n, first_bad


def bound(n, sumsq_ref):
    return n * U * sumsq_ref


def norm_of(sumsq_value):
    """fl32 of the f64 root"""
    with np.errstate(over="ignore"):
        return F32(np.sqrt(np.float64(sumsq_value)))


def decide(sumsq_value, any_bad, max_norm, skip_nonfinite):
    """-> (norm, nonfinite, skip, coef) from a sum of squares (the reference's, or the bits the device wrote)"""
    norm = norm_of(sumsq_value)
    nonfinite = bool(any_bad) or not np.isfinite(norm)
    skip = nonfinite and bool(skip_nonfinite)
    if skip:
        coef = F32(0.0)
    elif F32(max_norm) > 0 and not nonfinite:
        coef = min(F32(1.0), F32(max_norm) / (norm + F32(1e-6)))          # fp32 add, fp32 divide, both correctly rounded
    else:
        coef = F32(1.0)
    return norm, nonfinite, skip, F32(coef)


# ---- shared cases ------------------------------------------------------------------------------------------------------------
def values(kind, n, seed=0):
    rng = np.random.default_rng(seed + 7919 * n)
    if kind == "randn":
        return rng.standard_normal(n).astype(F32)
    if kind == "mixed":          # magnitudes spread over 1e-30 .. 1e18, both signs
        return (np.sign(rng.standard_normal(n)) * 10.0 ** rng.uniform(-30, 18, n)).astype(F32)
    if kind == "big":            # the square overflows fp32 and not fp64
        return np.full(n, 3e25, dtype=F32)
    raise ValueError(kind)


KINDS = ("randn", "mixed", "big")
SCALES = (1.0, 0.5)


def counts(chunk):
    return (0, 1, 3, 4, 5, 63, 64, 1003, chunk - 1, chunk, chunk + 1, 2 * chunk + 5)
