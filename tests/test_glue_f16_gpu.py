"""The fp16 outputs of the three glue kernels of the fp16 tower forward, through the C ABI, bit for bit: uniir_layernorm_fwd_f16 against
the bf16 entry point's own fp32 output, uniir_patchify_f16 / uniir_vit_assemble_f16 against the restatements of tests/glue_ref.py
applied with fp16 rounding.  Shapes: every LayerNorm register count (widths 64, 768, 1028), fewer and more rows than a block holds,
a patch grid of 2 x 2 and 3 x 3, a kpad above 3 P P."""
import pytest
import torch

import glue_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("width", [64, 768, 1028])
@pytest.mark.parametrize("rows", [3, 257])
def test_layernorm_fwd_f16_rounds_the_fp32_result_of_the_bf16_entry_point(rows, width):
    from uniir_amd import ops
    g = torch.Generator().manual_seed(rows * 10007 + width)
    x = (torch.randn(rows, width, generator=g) * 3 + 0.5).to(DEV)
    x[0, : width // 2] *= 1e3          # a row whose statistics are dominated by a few large elements
    gamma, beta = torch.randn(width, generator=g).to(DEV), torch.randn(width, generator=g).to(DEV)
    canary = 0x7B7B
    y16 = torch.full((rows + 1, width), canary, dtype=torch.int16, device=DEV).view(torch.float16)
    y32 = torch.empty(rows, width, device=DEV)
    ops.call("uniir_layernorm_fwd_f16", x, width, gamma, beta, y16, y32, rows, width, 1e-5)
    b16, b32 = torch.empty(rows, width, device=DEV, dtype=torch.bfloat16), torch.empty(rows, width, device=DEV)
    ops.call("uniir_layernorm_fwd", x, width, gamma, beta, b16, b32, rows, width, 1e-5)
    R.assert_bits(y32, b32, "y_f32 of the fp16 entry point against the bf16 entry point's")
    R.assert_bits(y16[:rows], y32.half(), "y_f16 against y_f32 rounded to fp16")
    assert bool((y16[rows].view(torch.int16) == canary).all())          # nothing behind the last row
    only16 = torch.empty(rows, width, device=DEV, dtype=torch.float16)          # each output alone
    ops.call("uniir_layernorm_fwd_f16", x, width, gamma, beta, only16, None, rows, width, 1e-5)
    R.assert_bits(only16, y16[:rows], "y_f16 alone")
    only32 = torch.empty(rows, width, device=DEV)
    ops.call("uniir_layernorm_fwd_f16", x, width, gamma, beta, None, only32, rows, width, 1e-5)
    R.assert_bits(only32, b32, "y_f32 alone")
    # the wrapper: an fp16 tensor in the 16-bit slot takes this entry point, dtype16 allocates one
    R.assert_bits(ops.layernorm_fwd(x, gamma, beta, out_bf16=torch.empty_like(only16), rows=rows, width=width), only16, "ops, given")
    R.assert_bits(ops.layernorm_fwd(x, gamma, beta, rows=rows, width=width, dtype16=torch.float16), only16, "ops, allocated")
    R.assert_bits(ops.layernorm_fwd(x, gamma, beta, rows=rows, width=width), b16, "ops, bf16 as before")


def _patch_rows_f16(img, P, kpad):
    """glue_ref.patchify with fp16 in place of its bf16 rounding"""
    n, ch, res, _ = img.shape
    g = res // P
    rows = img.reshape(n, ch, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, ch * P * P)
    out = torch.zeros(n * g * g, kpad, dtype=torch.float32, device=img.device)
    out[:, :ch * P * P] = rows
    return out.to(torch.float16)


@pytest.mark.parametrize("res", [32, 48])
@pytest.mark.parametrize("kpad", [768, 832])
def test_patchify_f16_and_vit_assemble_f16_equal_the_restatements_in_fp16(res, kpad):
    from uniir_amd import ops
    P, n, w = 16, 3, 64
    g = torch.Generator().manual_seed(res + kpad)
    img = (torch.randn(n, 3, res, res, generator=g) * 2).to(DEV)
    img[0, 0, 0, :4] = torch.tensor([70000.0, -70000.0, 1e-8, 65519.9])          # beyond fp16's range, below its subnormals, just under the last tie
    G = (res // P) ** 2
    canary = 0x7B7B
    patches = torch.full((n * G + 1, kpad), canary, dtype=torch.int16, device=DEV).view(torch.float16)
    ops.call("uniir_patchify_f16", img, patches, n, res, P, kpad)
    R.assert_bits(patches[:n * G], _patch_rows_f16(img, P, kpad), "fp16 patch rows")
    assert bool((patches[n * G].view(torch.int16) == canary).all())
    b = torch.empty(n * G, kpad, dtype=torch.bfloat16, device=DEV)
    ops.call("uniir_patchify", img, b, n, res, P, kpad)
    R.assert_bits(b, R.patchify(img, P, kpad), "bf16 patch rows, as before")
    T = G + 1
    po = (torch.randn(n * G, w, generator=g) * 4).to(DEV).half()
    cls, pos = torch.randn(w, generator=g).to(DEV), torch.randn(T, w, generator=g).to(DEV)
    x = torch.full((n * T + 1, w), 7.25, device=DEV)
    ops.call("uniir_vit_assemble_f16", po, cls, pos, x, n, T, w)
    R.assert_bits(x[:n * T], R.vit_assemble(po, cls, pos, n, T), "tokens assembled from an fp16 patch_out")
    assert bool((x[n * T] == 7.25).all())
