"""tests/attn_f32_rel_ref.py on the CPU: a numpy fp32 restatement of the evaluation order of uniir_attn_f32_rel_fwd stays inside the
derived bound of the fp64 reference (at half of it or less: the bound carries fp32_ref's MARGIN of 2), and each planted defect of the
bias addressing leaves it.  rel_emb is of order 1 and the defects are judged at scale 0.125, where the bias is as large as the
dot-product term, so every one of them moves logits by far more than the bound."""
import pytest
import torch

import attn_f32_rel_ref as R
from fp32_ref import worst_ratio

CASES = [(2, 2, 1), (2, 2, 31), (1, 2, 33), (1, 1, 70)]          # (batch, heads, seq): one key, a partial 32-key chunk on both sides, three chunks


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("batch,heads,seq", CASES)
def test_the_kernels_order_in_fp32_stays_inside_the_bound(batch, heads, seq, scale):
    qkv, emb, table = R.make_case(batch, heads, seq)
    ref, bound = R.reference(qkv, emb, table, scale, batch, seq, heads)
    got = R.kernel_order_f32(qkv, emb, table, scale, batch, seq, heads)
    assert ref.shape == bound.shape == got.shape == (batch * seq, heads * 64) and bool((bound > 0).all())
    ratio = worst_ratio(got, ref, bound)
    print(f"\nOBS attn_f32_rel restatement ({batch},{heads},{seq}) scale {scale}: worst ratio {ratio:.3f}, largest bound {float(bound.max()):.2e}")
    assert ratio <= 0.5, ratio


def test_the_reference_is_the_formula_written_out():
    """one output element by hand, in python floats, from the table and the embedding"""
    batch, heads, seq, scale = 1, 2, 5, 0.125
    qkv, emb, table = R.make_case(batch, heads, seq, seed=3)
    ref, _ = R.reference(qkv, emb, table, scale, batch, seq, heads)
    x = qkv.double().view(seq, 3, heads, 64)
    i, h = 3, 1
    logits = [scale * float(x[i, 0, h] @ x[j, 1, h]) + float(emb[int(table[j - i + seq - 1]), h]) for j in range(seq)]
    w = torch.softmax(torch.tensor(logits, dtype=torch.float64), 0)
    want = sum(w[j] * x[j, 2, h] for j in range(seq))
    assert torch.allclose(ref[i, h * 64:(h + 1) * 64], want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("batch,heads,seq,defect", [c + (d,) for c in CASES[1:] for d in R.DEFECTS if d != "head_swapped" or c[1] > 1])
def test_each_planted_defect_leaves_the_bound(batch, heads, seq, defect):
    scale = 0.125
    qkv, emb, table = R.make_case(batch, heads, seq)
    ref, bound = R.reference(qkv, emb, table, scale, batch, seq, heads)
    got = R.kernel_order_f32(qkv, emb, table, scale, batch, seq, heads, defect=defect)
    ratio = worst_ratio(got, ref, bound)
    print(f"\nOBS attn_f32_rel defect {defect} ({batch},{heads},{seq}): worst ratio {ratio:.3e}")
    assert ratio > 100.0, (defect, ratio)
