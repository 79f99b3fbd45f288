"""The streaming attention kernels (csrc/attention_long.hip): plain self-attention of 513 .. 1024 tokens, forward and backward in bf16,
against fp32 torch on the bf16-rounded inputs (the reference of tests/test_kernels_gpu.py::test_attention_fwd_bwd, restated here),
with that test's gates.

The fp16 forward (attn_long_fwd_kernel<true>) has its own entry point, uniir_attention_fwd_f16: tests/test_attention_paths_gpu.py
judges it element by element against the fp64 reference at 513 .. 1024 tokens, and the fp16 towers reach it in
tests/test_clip_336_gpu.py::test_fp16_and_fp32_embeddings_against_the_oracle (577 tokens, against the fp32 oracle)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))

DEV = "cuda"


def _ops():
    from uniir_amd import ops
    return ops


def rel_err(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / (b.norm() + 1e-12)).item()


def bf(x):
    return x.to(torch.bfloat16)


def _attn_ref(qkv, batch, seq, heads):
    W = heads * 64
    q, k, v = qkv.float().view(batch, seq, 3, heads, 64).permute(2, 0, 3, 1, 4)
    s = (q @ k.transpose(-1, -2)) * 0.125
    p = torch.softmax(s, -1)
    o = (p @ v).permute(0, 2, 1, 3).reshape(batch * seq, W)
    return o, torch.logsumexp(s, -1)


def _run(qkv, do, batch, seq, heads):
    """forward and backward into sentinel-filled buffers; every element must have been written with a finite value"""
    ops = _ops()
    W = heads * 64
    out = torch.full((batch * seq, W), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((batch, heads, seq), float("nan"), device=DEV, dtype=torch.float32)
    ops.attention_fwd(qkv, batch, seq, heads, 0, out=out, lse=lse)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse).all())
    dqkv = torch.full_like(qkv, float("nan"))
    ops.attention_bwd(qkv, out, do, lse, batch, seq, heads, 0, dqkv=dqkv)
    assert bool(torch.isfinite(dqkv.float()).all())
    return out, lse, dqkv


def _check(qkv, do, out, lse, dqkv, batch, seq, heads, lse_gate=True):
    W = heads * 64
    qr = qkv.float().requires_grad_(True)
    oref, lref = _attn_ref(qr, batch, seq, heads)
    e = rel_err(out, oref.detach())
    print("OBS long attention", (batch, seq, heads), "out", e, "lse", float((lse - lref.detach()).abs().max()))
    assert e < 8e-3, e
    if lse_gate:
        assert (lse - lref.detach()).abs().max() < 2e-3
    oref.backward(do.float())
    g = qr.grad.view(batch * seq, 3, W)
    d = dqkv.float().view(batch * seq, 3, W)
    for i, name in enumerate("qkv"):
        e = rel_err(d[:, i], g[:, i])
        print("OBS long attention", (batch, seq, heads), "d" + name, e)
        assert e < 1.5e-2, (name, e)


# 513: one live row past the old limit; 577: ViT-L/14@336px, 36 tiles + 1; 529: the last 128-row chunk holds one 16-row tile + 1 row;
# 640: no tail; 1024: the maximum; several items and heads for the grid indexing
@pytest.mark.parametrize("batch,seq,heads", [(1, 513, 3), (2, 577, 2), (3, 529, 1), (2, 640, 1), (1, 1024, 2)])
def test_long_attention_fwd_bwd(batch, seq, heads):
    torch.manual_seed(5)
    W = heads * 64
    qkv = bf(torch.randn(batch * seq, 3 * W, device=DEV))
    do = bf(torch.randn(batch * seq, W, device=DEV))
    out, lse, dqkv = _run(qkv, do, batch, seq, heads)
    _check(qkv, do, out, lse, dqkv, batch, seq, heads)


@pytest.mark.parametrize("seq", [577, 1024])
def test_long_attention_rescale_path(seq):
    """the running maximum of a row jumps late (query 5 meets its spiking key seq - 17 in the last chunk) and early (query seq - 2 meets
    key 3 in the first): one head, queries scaled by 0.1 so that nothing else moves the reference far"""
    torch.manual_seed(9)
    x = torch.randn(seq, 3, 64, device=DEV)
    x[:, 0] *= 0.1
    x[seq - 17, 1] = 400.0 * x[5, 0]
    x[3, 1] = 400.0 * x[seq - 2, 0]
    qkv = bf(x.reshape(seq, 192))
    do = bf(torch.randn(seq, 64, device=DEV))
    out, lse, dqkv = _run(qkv, do, 1, seq, 1)
    _check(qkv, do, out, lse, dqkv, 1, seq, 1, lse_gate=False)


def test_long_attention_is_reproducible():
    torch.manual_seed(2)
    batch, seq, heads = 2, 577, 2
    qkv = bf(torch.randn(batch * seq, 3 * heads * 64, device=DEV))
    do = bf(torch.randn(batch * seq, heads * 64, device=DEV))
    a = _run(qkv, do, batch, seq, heads)
    b = _run(qkv, do, batch, seq, heads)
    for x, y, name in zip(a, b, ("out", "lse", "dqkv")):
        assert torch.equal(x, y), name


def test_long_attention_rows_are_independent():
    """rows 0 .. 15 of a 577-token call do not change when the queries of every other row are replaced by noise (K / V untouched)"""
    ops = _ops()
    torch.manual_seed(3)
    batch, seq, heads = 2, 577, 2
    W = heads * 64
    qkv = bf(torch.randn(batch * seq, 3 * W, device=DEV))
    other = qkv.clone().view(batch, seq, 3 * W)
    other[:, 16:, :W] = bf(torch.randn(batch, seq - 16, W, device=DEV) * 3.0)
    other = other.view(batch * seq, 3 * W).contiguous()
    o1, l1 = ops.attention_fwd(qkv, batch, seq, heads, 0)
    o2, l2 = ops.attention_fwd(other, batch, seq, heads, 0)
    assert torch.equal(o1.view(batch, seq, W)[:, :16], o2.view(batch, seq, W)[:, :16])
    assert torch.equal(l1[:, :, :16], l2[:, :, :16])
    assert not torch.equal(o1.view(batch, seq, W)[:, 16:], o2.view(batch, seq, W)[:, 16:])


def test_long_attention_limits_through_the_c_abi():
    from uniir_amd import _lib
    ops = _ops()
    lib = _lib.load()
    heads, cap = 1, 1025
    qkv = bf(torch.randn(cap, 192, device=DEV))
    out = torch.empty(cap, 64, device=DEV, dtype=torch.bfloat16)
    do = bf(torch.randn(cap, 64, device=DEV))
    lse = torch.empty(cap, device=DEV, dtype=torch.float32)
    dqkv = torch.empty_like(qkv)
    p = ops._p

    def fwd(seq, causal):
        return lib.uniir_attention_fwd(p(qkv), p(out), p(lse), 1, seq, heads, causal, ops._stream())

    def bwd(seq, causal):
        return lib.uniir_attention_bwd(p(qkv), p(out), p(do), p(lse), p(dqkv), 1, seq, heads, causal, ops._stream())

    assert fwd(1025, 0) == -2 and bwd(1025, 0) == -2
    assert fwd(600, 1) == -2 and bwd(600, 1) == -2
    for seq in (512, 513):
        assert fwd(seq, 0) == 0
        assert bwd(seq, 0) == 0
    torch.cuda.synchronize()
