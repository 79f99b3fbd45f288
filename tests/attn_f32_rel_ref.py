"""fp64 reference of uniir_attn_f32_rel_fwd (csrc/fp32_path.hip: fp32 self-attention with the T5 relative-position bias) and an
element-wise error bound derived from the kernel's arithmetic, the way tests/fp32_ref.py derives its bounds (EPS32, gamma, the device
math budgets and MARGIN are that module's).

Not a test module: tests/test_attn_f32_rel_gpu.py compares the kernel with it, tests/test_attn_f32_rel_ref.py checks on the CPU that a
numpy fp32 restatement of the kernel's evaluation order stays inside the bound and that planted defects do not.

The formula (include/uniir_hip.h): qkv [batch*seq, 3*heads*64] packed q | k | v, per (item, head)
    logit(i, j) = scale * <q_i, k_j> + rel_emb[rel_bucket[j - i + seq - 1]][head],   out_i = sum_j softmax_j(logit(i, .)) v_j.

The bound, per output element (i, d), n = seq keys:
  logit.   The kernel rounds q_d * scale once, runs one 64-term fmaf chain and adds the bias with one rounding.  With A_ij =
           sum_d |scale q_id k_jd| and b_ij the bias:  e_s(i, j) = gamma(66) (A_ij + |b_ij|)     (65 roundings on the products, one on the sum
           s + b, whose magnitude is at most A + |b|).
  weights. Online softmax: key j enters with p = exp(s_j - m) under the running maximum m and is multiplied by alpha = exp(m - m')
           whenever the maximum moves afterwards; alpha is exp(0) = 1, exactly, when it does not.  The exact factors telescope to
           exp(s_j - M) for the final maximum M, which every key shares (a softmax does not see a common shift).  With c_i the number of
           times row i's running maximum moves and span_i = max_j s - min_j s, key j's weight has the relative error
               rho_ij = e_s(i, j) + (c_i + 1) (R_EXP + 2 EPS32) + 2 EPS32 span_i
           (one exp budget and one product per factor; the subtractions' roundings are relative to arguments that add up to at most
           twice the span).  First order in e_s: the margin covers the second.
  sums.    acc_d = fmaf(p, v_jd, acc_d * alpha) and l = l * alpha + p over the n keys in order: every term passes through at most n
           additions and c_i inexact products, G_i = gamma(n + c_i + 2).
  output.  out = acc * (1 / l): R_DIV + 2 EPS32.  With P = softmax, relative errors r_j of the weights move the output by
           sum_j P_ij r_j (v_jd - out_id) to first order (a common factor of all weights cancels; one key has nothing to move):
               |out^ - out|_id <= sum_j P_ij rho_ij |v_jd - out_id| + G_i (sum_j P_ij |v_jd| + |out_id|) + |out_id| (R_DIV + 2 EPS32)
Every bound is MARGIN times that, plus TINY32."""
import numpy as np
import torch

from fp32_ref import EPS32, MARGIN, R_DIV, R_EXP, TINY32, gamma

DEFECTS = ("offset_plus_one", "transposed_offset", "bias_times_scale", "bias_missing", "head_swapped")


def _split(qkv, batch, seq, heads):
    """packed [batch*seq, 3*heads*64] -> q, k, v [batch, heads, seq, 64]"""
    x = qkv.view(batch, seq, 3, heads, 64).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def _bias(rel_emb, table, seq):
    """[heads, seq, seq]: rel_emb[table[j - i + seq - 1]][head]"""
    pos = torch.arange(seq)
    idx = pos[None, :] - pos[:, None] + seq - 1
    return rel_emb[table.long()[idx]].permute(2, 0, 1)


def reference(qkv, rel_emb, table, scale, batch, seq, heads):
    """-> (out float64 [batch*seq, heads*64], bound float64 of the same shape)"""
    q, k, v = _split(qkv.double(), batch, seq, heads)
    b = _bias(rel_emb.double(), table, seq)[None]
    s = scale * (q @ k.transpose(-1, -2)) + b
    P = torch.softmax(s, dim=-1)
    out = P @ v
    A = abs(scale) * (q.abs() @ k.abs().transpose(-1, -2))
    e_s = gamma(66) * (A + b.abs())
    cm = s.cummax(-1).values
    c = (cm[..., 1:] > cm[..., :-1]).sum(-1, keepdim=True).double() + 1          # moves of the running maximum, the first key included
    span = (s.max(-1, keepdim=True).values - s.min(-1, keepdim=True).values)
    rho = e_s + (c + 1) * (R_EXP + 2 * EPS32) + 2 * EPS32 * span
    n = torch.full_like(c, float(seq)) + c + 2
    G = n * EPS32 / (1.0 - n * EPS32)
    w = P * rho
    moved = torch.cat([(w[:, :, i0:i0 + 64, :, None] * (v[:, :, None, :, :] - out[:, :, i0:i0 + 64, None, :]).abs()).sum(-2)
                       for i0 in range(0, seq, 64)], dim=2)          # sum_j P rho |v_j - out_i|, 64 query rows at a time
    bound = moved + G * (P @ v.abs() + out.abs()) + out.abs() * (R_DIV + 2 * EPS32)
    bound = MARGIN * bound + TINY32
    flat = lambda t: t.permute(0, 2, 1, 3).reshape(batch * seq, heads * 64)          # noqa: E731
    return flat(out), flat(bound)


def _fma32(a, b, c):
    """fl32(a * b + c) of fp32 arrays: the product of two fp32 numbers is exact in fp64; the sum is rounded to fp64, then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def kernel_order_f32(qkv, rel_emb, table, scale, batch, seq, heads, defect=None):
    """numpy fp32 restatement of the kernel's evaluation order (scale folded into q, one fmaf chain in ascending d, the bias added
    after the chain, online softmax over the keys in order) -> fp32 [batch*seq, heads*64].  defect: one of DEFECTS, planted."""
    f32 = np.float32
    q, k, v = (t.contiguous().numpy().astype(f32) for t in _split(qkv.float(), batch, seq, heads))
    emb, tab = rel_emb.numpy().astype(f32), table.numpy().astype(np.int64)
    pos = np.arange(seq)
    off = pos[None, :] - pos[:, None] + seq - 1
    if defect == "offset_plus_one":
        off = np.minimum(off + 1, 2 * seq - 2)
    elif defect == "transposed_offset":
        off = off.T
    elif defect not in (None, "bias_times_scale", "bias_missing", "head_swapped"):
        raise ValueError(defect)
    bias = np.transpose(emb[tab[off]], (2, 0, 1))                                   # [heads, seq, seq]
    if defect == "head_swapped":
        bias = bias[::-1]
    if defect == "bias_times_scale":
        bias = (bias * f32(scale)).astype(f32)
    qs = (q * f32(scale)).astype(f32)
    s = np.zeros((batch, heads, seq, seq), f32)
    for d in range(64):
        s = _fma32(qs[..., :, None, d], k[..., None, :, d], s)
    if defect != "bias_missing":
        s = (s + bias[None]).astype(f32)
    mx = np.full((batch, heads, seq), -np.inf, f32)
    l = np.zeros((batch, heads, seq), f32)
    acc = np.zeros((batch, heads, seq, 64), f32)
    with np.errstate(invalid="ignore"):
        for j in range(seq):
            mn = np.maximum(mx, s[..., j])
            alpha, p = np.exp(mx - mn).astype(f32), np.exp(s[..., j] - mn).astype(f32)
            l = ((l * alpha).astype(f32) + p).astype(f32)
            acc = _fma32(p[..., None], v[:, :, j, None, :], (acc * alpha[..., None]).astype(f32))
            mx = mn
    out = (acc * (f32(1.0) / l)[..., None]).astype(f32)
    return torch.from_numpy(np.transpose(out, (0, 2, 1, 3)).reshape(batch * seq, heads * 64).copy())


def make_case(batch, heads, seq, seed=0, emb_std=1.0):
    """seeded inputs: qkv of order 1 (logits of standard deviation 8 at scale 1, 1 at scale 0.125), rel_emb of order 1 (32 buckets)
    and the bucket table of the CLIP_FF stack -> qkv fp32 [batch*seq, 3*heads*64], rel_emb fp32 [32, heads], table int32 [2 seq - 1]"""
    from uniir_amd.clipff_model import T5_BUCKETS, rel_bucket_table
    g = torch.Generator().manual_seed(1000 * seed + 7 * seq + heads)
    qkv = torch.randn(batch * seq, 3 * heads * 64, generator=g)
    rel_emb = torch.randn(T5_BUCKETS, heads, generator=g) * emb_std
    return qkv, rel_emb, rel_bucket_table(seq)
