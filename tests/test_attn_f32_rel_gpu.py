"""uniir_attn_f32_rel_fwd (csrc/fp32_path.hip) on the device: fp32 self-attention with the T5 relative-position bias against the fp64
reference of tests/attn_f32_rel_ref.py, inside its derived bound; with an all-zero rel_emb the bits of uniir_attention_f32_fwd on the
same packed buffer (the two entry points are two instantiations of one kernel body); the refusals, each with its code and an untouched
output.

Shapes (batch, heads, seq): one key; 31 / 33 on both sides of a 32-key chunk; 257 = a second 256-row pass with a one-row tail; 654 =
the workload's largest (ViT-L/14@336px: 77 + 577 fused tokens).  32 buckets with clipff_model.rel_bucket_table, scale 1 (the T5 stack)
and 0.125."""
import ctypes as C

import pytest
import torch

import attn_f32_rel_ref as R
from fp32_ref import worst_ratio

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2, 1), (2, 2, 31), (1, 2, 33), (2, 1, 257), (1, 1, 654)]
OK, EINVAL, ESHAPE = 0, -1, -2
_REF = {}


def _reference(batch, heads, seq, scale):
    """the case and its fp64 reference, computed once per (shape, scale) and left unchanged"""
    key = (batch, heads, seq, scale)
    if key not in _REF:
        case = R.make_case(batch, heads, seq)
        _REF[key] = case + R.reference(*case, scale, batch, seq, heads)
    return _REF[key]


def _run(qkv, emb, table, scale, batch, seq, heads):
    from uniir_amd import ops
    out = torch.full((batch * seq, heads * 64), float("nan"), device="cuda")
    ops.call("uniir_attn_f32_rel_fwd", qkv.cuda(), out, emb.cuda(), table.cuda(), int(emb.shape[0]), float(scale), batch, seq, heads)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("scale", [1.0, 0.125])
@pytest.mark.parametrize("batch,heads,seq", SHAPES)
def test_inside_the_derived_bound_of_the_fp64_reference(batch, heads, seq, scale):
    qkv, emb, table, ref, bound = _reference(batch, heads, seq, scale)
    got = _run(qkv, emb, table, scale, batch, seq, heads).cpu()
    ratio = worst_ratio(got, ref, bound)
    print(f"\nOBS uniir_attn_f32_rel_fwd ({batch},{heads},{seq}) scale {scale}: worst |got - ref| / bound {ratio:.3f}, "
          f"max |got - ref| {float((got.double() - ref).abs().max()):.2e}")
    assert ratio <= 1.0, ratio


@pytest.mark.parametrize("batch,heads,seq", SHAPES)
def test_a_zero_bias_has_the_bits_of_the_entry_point_without_bias(batch, heads, seq):
    from uniir_amd import ops
    qkv, emb, table = R.make_case(batch, heads, seq, seed=1)
    W = heads * 64
    for scale in (1.0, 0.125):
        got = _run(qkv, torch.zeros_like(emb), table, scale, batch, seq, heads)
        dq = qkv.cuda()
        want = torch.full_like(got, float("nan"))
        ops.call("uniir_attention_f32_fwd", dq, 3 * W, dq[:, W:], dq[:, 2 * W:], 3 * W, want, W, None, batch, seq, seq, heads, 0, float(scale))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(want).all()) and torch.equal(got, want), (scale, float((got - want).abs().max()))
    if seq > 1:          # and the bias is not ignored: the same call with the embedding moves the output
        assert not torch.equal(_run(qkv, emb, table, 1.0, batch, seq, heads), got)


def test_refused_calls_return_their_code_and_write_nothing():
    from uniir_amd import _lib
    lib = _lib.load()
    batch, heads, seq = 2, 2, 8
    qkv, emb, table = (t.cuda() for t in R.make_case(batch, heads, seq))
    out = torch.full((batch * seq, heads * 64), 7.5, device="cuda")
    good = dict(qkv=qkv.data_ptr(), out=out.data_ptr(), rel_emb=emb.data_ptr(), rel_bucket=table.data_ptr(), nbuckets=32, scale=1.0,
                batch=batch, seq=seq, heads=heads)
    rows = [({p: None}, EINVAL) for p in ("qkv", "out", "rel_emb", "rel_bucket")]
    rows += [({"heads": 0}, EINVAL), ({"heads": -1}, EINVAL), ({"batch": -1}, EINVAL), ({"nbuckets": 0}, EINVAL), ({"nbuckets": 65}, EINVAL),
             ({"seq": 0}, ESHAPE), ({"seq": -3}, ESHAPE), ({"seq": 1025}, ESHAPE), ({"batch": 0}, OK), ({"batch": 0, "seq": 0}, OK)]
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for change, code in rows:
        a = {**good, **change}
        got = lib.uniir_attn_f32_rel_fwd(a["qkv"], a["out"], a["rel_emb"], a["rel_bucket"], a["nbuckets"], a["scale"], a["batch"], a["seq"],
                                         a["heads"], stream)
        torch.cuda.synchronize()
        assert got == code, (change, got, code)
        assert bool((out == 7.5).all()), change
    assert lib.uniir_attn_f32_rel_fwd(*[good[k] for k in ("qkv", "out", "rel_emb", "rel_bucket", "nbuckets", "scale", "batch", "seq", "heads")],
                                      stream) == OK
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.5).any())
