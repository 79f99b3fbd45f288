"""ops.linear_dgrad on 128-tile problems, where uniir_gemm itself runs the act(aux) pass before the product and the column-sum pass
after it: out, act_out and colsum must equal, bit for bit, the explicit sequence uniir_act_fwd -> uniir_gemm without C2 / colsum ->
uniir_colsum_bf16 that the Python layer ran itself before the library took both passes over."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (M, out features, in features): M < 256 twice, a reduction length that is no multiple of 64 once -> the 128 x 128 kernel
SHAPES = [(200, 136, 200), (248, 392, 192), (264, 120, 128)]
VARIANTS = [(), ("aux",), ("aux", "act_out"), ("aux", "act_out", "colsum"), ("colsum",)]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("case", range(len(SHAPES)))
def test_linear_dgrad_equals_the_explicit_pass_sequence(case):
    from uniir_amd import ops
    M, fo, fi = SHAPES[case]
    act = (ops.ACT_QUICKGELU, ops.ACT_GELU_ERF, ops.ACT_RELU)[case]
    g = torch.Generator(device=DEV).manual_seed(100 + case)
    dy = torch.randn(M, fo, device=DEV, generator=g).bfloat16()
    w = (torch.randn(fo, fi, device=DEV, generator=g) * fo ** -0.5).bfloat16()
    pre = torch.randn(M, fi, device=DEV, generator=g).bfloat16()
    colsum0 = torch.randn(fi, device=DEV, generator=g)
    for variant in VARIANTS:
        aux = pre if "aux" in variant else None
        want_out = torch.empty(M, fi, device=DEV, dtype=torch.bfloat16)
        want_act = torch.full((M, fi), -1.0, device=DEV, dtype=torch.bfloat16) if "act_out" in variant else None
        want_sum = colsum0.clone() if "colsum" in variant else None
        if want_act is not None:
            ops.call("uniir_act_fwd", aux, want_act, aux.numel(), act)
        ops.gemm(dy, w, want_out, M, fi, fo, fo, fi, fi, b_tmaj=True, epilogue=ops.EPI_DACT if aux is not None else ops.EPI_BF16,
                 aux=aux, ldaux=fi, act=act)
        if want_sum is not None:
            ops.call("uniir_colsum_bf16", want_out, fi, want_sum, M, fi)
        got_act = torch.full_like(want_act, -2.0) if want_act is not None else None
        got_sum = colsum0.clone() if want_sum is not None else None
        got_out = ops.linear_dgrad(dy, w, aux=aux, act=act, act_out=got_act, colsum=got_sum)
        torch.cuda.synchronize()
        assert torch.equal(_bits(got_out), _bits(want_out)), (variant, "out")
        assert float(want_out.float().abs().max()) > 0.1, variant          # the product ran
        if want_act is not None:
            assert torch.equal(_bits(got_act), _bits(want_act)), (variant, "act_out")
        if want_sum is not None:
            assert torch.equal(_bits(got_sum), _bits(want_sum)), (variant, "colsum")
            assert not torch.equal(got_sum, colsum0), variant          # ... and the sums were added to the vector
