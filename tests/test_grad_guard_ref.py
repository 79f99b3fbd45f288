"""CPU checks of tests/grad_guard_ref.py itself: the bound holds for honest fp64 restatements in any order and catches the two
mistakes a kernel of this kind makes (an fp32 accumulator, a forgotten tail); the coefficient formula at its edges."""
import numpy as np
import pytest

import grad_guard_ref as G

CHUNK = 65536          # any chunking does for the restatements; the library's own constant is read in the GPU tests


def _fp64_chunked(g, scale, chunk=CHUNK, perm=None, acc=np.float64, drop_tail=False):
    """the kernel's shape in numpy: per-chunk partials in `acc` precision, then the partials; optionally permuted, optionally
    forgetting the count % 4 tail"""
    x = G.scaled(g, scale)
    x = np.where(np.isfinite(x), x, G.F32(0))
    if drop_tail:
        x = x[:x.size // 4 * 4]
    if perm is not None:
        x = x[perm[perm < x.size]]
    total = acc(0)
    with np.errstate(over="ignore"):
        for lo in range(0, x.size, chunk):
            part = acc(0)
            c = x[lo:lo + chunk].astype(acc)
            for lane in range(4):          # four strided accumulators, added pairwise
                part = acc(part + (c[lane::4] * c[lane::4]).sum(dtype=acc))
            total = acc(total + part)
    return float(total)


@pytest.mark.parametrize("kind", G.KINDS)
@pytest.mark.parametrize("scale", G.SCALES)
@pytest.mark.parametrize("n", [1, 5, 1003, CHUNK + 1, 2 * CHUNK + 5])
def test_fp64_restatement_in_a_permuted_order_stays_inside_the_bound(kind, scale, n):
    g = G.values(kind, n)
    ref, cnt, bad = G.sumsq(g, scale)
    assert cnt == n and bad is None
    perm = np.random.default_rng(1).permutation(n)
    for got in (_fp64_chunked(g, scale), _fp64_chunked(g, scale, perm=perm), _fp64_chunked(g, scale, chunk=1000)):
        assert abs(got - ref) <= G.bound(n, ref)


def test_planted_fp32_accumulator_violates_the_bound():
    n = 2 * CHUNK + 5
    g = G.values("big", n)          # 3e25: the squares overflow fp32 and not fp64
    ref, _, _ = G.sumsq(g, 1.0)
    assert np.isfinite(ref) and abs(_fp64_chunked(g, 1.0) - ref) <= G.bound(n, ref)
    got = _fp64_chunked(g, 1.0, acc=np.float32)
    assert not abs(got - ref) <= G.bound(n, ref)
    g = G.values("randn", n)        # and without any overflow an fp32 sum is still far outside
    ref, _, _ = G.sumsq(g, 1.0)
    assert not abs(_fp64_chunked(g, 1.0, acc=np.float32) - ref) <= G.bound(n, ref)


@pytest.mark.parametrize("n", [1003, 5, CHUNK + 1])
def test_planted_forgotten_tail_violates_the_bound(n):
    g = G.values("randn", n)
    ref, _, _ = G.sumsq(g, 0.5)
    assert abs(_fp64_chunked(g, 0.5) - ref) <= G.bound(n, ref)
    assert not abs(_fp64_chunked(g, 0.5, drop_tail=True) - ref) <= G.bound(n, ref)


def test_nonfinite_elements_add_nothing_and_are_located():
    g = G.values("randn", 1003)
    for bad in (np.nan, np.inf, -np.inf):
        h = g.copy()
        h[77] = bad
        h[900] = bad
        ref, n, first = G.sumsq([g[:10], h], 1.0)
        clean, _, _ = G.sumsq([g[:10], np.delete(h, [77, 900])], 1.0)
        assert first == (1, 77) and n == 1013 and ref == clean
    # a finite g whose scaled value overflows is non-finite too: x is what AdamW consumes
    assert G.sumsq(np.array([3e38], dtype=G.F32), 2.0)[2] == (0, 0)


def test_coefficient_formula_edges():
    F = G.F32
    # norm = 0: the quotient is huge, the coefficient 1
    assert G.decide(0.0, False, 1.0, False) == (F(0), False, False, F(1))
    # norm = max_norm: max_norm / (norm + 1e-6) is just below 1, as torch's clip_grad_norm_ gives
    norm, nonfinite, skip, coef = G.decide(4.0, False, 2.0, False)
    assert norm == F(2) and coef == F(2) / (F(2) + F(1e-6)) and coef < 1 and not nonfinite and not skip
    # above: clipped; far below: 1; max_norm <= 0: off
    assert G.decide(100.0, False, 2.0, False)[3] == F(2) / (F(10) + F(1e-6))
    assert G.decide(1e-8, False, 2.0, False)[3] == F(1)
    assert G.decide(100.0, False, 0.0, False)[3] == F(1) and G.decide(100.0, False, -1.0, False)[3] == F(1)
    # norm overflows fp32 (sumsq finite in fp64): non-finite; the coefficient stays 1 unless the step is skipped, then 0
    norm, nonfinite, skip, coef = G.decide(1e79, False, 2.0, False)
    assert np.isinf(norm) and nonfinite and not skip and coef == F(1)
    assert G.decide(1e79, False, 2.0, True)[1:] == (True, True, F(0))
    # a non-finite element with a finite norm: no clipping either
    assert G.decide(100.0, True, 2.0, False)[1:] == (True, False, F(1))
    assert G.decide(100.0, True, 0.0, True)[1:] == (True, True, F(0))
