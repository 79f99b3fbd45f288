"""CPU test of the fp64 GEMM reference and its bound (tests/gemm_ref.py): a result computed the way the kernels compute it passes,
and results with one wrong edge element, a bias added twice, a transposed tile or a wrong column / row sum fail."""
import pytest
import torch

import gemm_ref as R


def _problem(M=40, N=48, K=96, seed=0, dtype=torch.bfloat16):
    g = torch.Generator().manual_seed(seed)
    A = R.round16(torch.randn(M, K, generator=g, dtype=torch.float64), dtype)
    B = R.round16(torch.randn(K, N, generator=g, dtype=torch.float64), dtype)
    bias = torch.randn(N, generator=g, dtype=torch.float64).float()
    return A, B, bias


def _emulate(A, B, bias, alpha, out):
    """what the kernel computes: exact products, fp32 sums, fp32 epilogue, rounded output"""
    v = (A.float() @ B.float()) * alpha + bias
    return v.to(out)


@pytest.mark.parametrize("out", [torch.float32, torch.bfloat16, torch.float16])
def test_reference_accepts_a_correct_result_and_rejects_corrupted_ones(out):
    dt = torch.float16 if out == torch.float16 else torch.bfloat16
    A, B, bias = _problem(dtype=dt)
    alpha = -3.0
    epi = R.EPI_F32 if out == torch.float32 else R.EPI_BF16
    ref = R.gemm_reference(A, B, epilogue=epi, alpha=alpha, bias=bias, out16=out if out != torch.float32 else torch.bfloat16)
    C, bound = ref["C"]
    good = _emulate(A, B, bias, alpha, out)
    R.check(good, C, bound, "correct")
    absab = abs(alpha) * (A.abs() @ B.abs())
    M, N = good.shape

    edge = good.double().clone()           # one edge element off by 1 % of |A||B|
    edge[M - 1, N - 1] += 0.01 * absab[M - 1, N - 1]
    edge = edge.to(out)
    assert bool(R.violations(edge, C, bound).any())
    edge0 = good.double().clone()
    edge0[0, N - 1] -= 0.01 * absab[0, N - 1]
    assert bool(R.violations(edge0.to(out), C, bound).any())

    twice = (good.double() + bias.double()).to(out)      # the bias added twice
    assert bool(R.violations(twice, C, bound).any())

    tr = good.clone()                      # one 16 x 16 tile transposed
    tr[16:32, 16:32] = good[16:32, 16:32].t()
    assert bool(R.violations(tr, C, bound).any())

    nan = good.clone()
    nan[M // 2, 3] = float("nan")
    assert bool(R.violations(nan, C, bound).any())
    with pytest.raises(AssertionError):
        R.check(tr, C, bound, "transposed tile")


def test_column_and_row_sums_reject_corruption():
    A, B, bias = _problem(M=64, N=32, K=200, seed=1)
    cs0 = torch.randn(N := 32, dtype=torch.float64).float()
    rs0 = torch.randn(64, dtype=torch.float64).float()
    ref = R.gemm_reference(A, B, epilogue=R.EPI_F32, alpha=0.5, bias=bias, colsum0=cs0, rowsum0=rs0)
    v = (A.float() @ B.float()) * 0.5 + bias
    R.check(v, *ref["C"], "C")
    cs = cs0 + v.sum(0)
    rs = rs0 + A.float().sum(1)
    R.check(cs, *ref["colsum"], "colsum")
    R.check(rs, *ref["rowsum"], "rowsum")
    absab = 0.5 * (A.abs() @ B.abs())
    bad = cs.clone()
    bad[N - 1] += 0.01 * float(absab[:, N - 1].max())     # one row's term 1 % off
    assert bool(R.violations(bad, *ref["colsum"]).any())
    assert bool(R.violations(cs + bias, *ref["colsum"]).any())          # the bias counted once more per column
    assert bool(R.violations(rs * 0.5, *ref["rowsum"]).any())           # a row sum scaled by alpha
    assert bool(R.violations(cs0 + 2 * v.sum(0), *ref["colsum"]).any())  # partials added twice


@pytest.mark.parametrize("act", [R.ACT_QUICKGELU, R.ACT_GELU_ERF, R.ACT_RELU])
def test_activation_epilogues(act):
    A, B, bias = _problem(seed=2 + act)
    A = A / 8
    f = _emulate(A, B, bias, 1.0, torch.bfloat16)
    ref = R.gemm_reference(A, B, epilogue=R.EPI_BIAS_ACT, bias=bias, act=act, got_f=f)
    R.check(f, *ref["C"], "f")
    g = R.act_fwd(f.double(), act).float().to(torch.bfloat16)
    R.check(g, *ref["C2"], "act(f)")
    assert bool(R.violations(f, *ref["C2"]).any()) or act == R.ACT_RELU and bool((f >= 0).all())
    only = R.gemm_reference(A, B, epilogue=R.EPI_ACT_ONLY, bias=bias, act=act)
    R.check(g, *only["C"], "act only")
    aux = R.round16(torch.randn(f.shape, dtype=torch.float64), torch.bfloat16)
    d = R.gemm_reference(A, B, epilogue=R.EPI_DACT, bias=bias, act=act, aux=aux)
    dx = ((A.float() @ B.float() + bias) * R.act_bwd(aux, act).float()).to(torch.bfloat16)
    R.check(dx, *d["C"], "dact")
    assert bool(R.violations(((A.float() @ B.float()) * R.act_bwd(aux, act).float()).to(torch.bfloat16), *d["C"]).any())
