"""fp64 reference of the fused attention kernels (include/uniir_hip.h, [ENC] building block 3 and uniir_attention_rel_*), an
element-wise error bound derived from their arithmetic, an fp32 emulator of that arithmetic, and mutations.

Not a test module: tests/test_attention_paths_gpu.py compares every kernel path against the reference and
tests/test_attention_ref.py checks on the CPU that the emulator fits the bound and that the bound rejects mutated results.
Everything is device-agnostic torch on ONE item: q [Tq][H][64], k / v [Tk][H][64], already rounded to the kernel's 16-bit type.

The operation.  s[h][i][j] = scale * q[i][h] . k[j][h] + bias[h][i][j]  (bias = rel_emb[rel_bucket[j - i + Tq - 1]][h] or 0);
key j is valid for query i when j < key_len and (not causal or j <= i);  lse[h][i] = log sum_valid exp(s);  p = exp(s - lse) on
valid keys, 0 elsewhere;  out[i][h] = sum_j p f v[j][h] with the dropout factors f (0 or 1 / keep; all 1 without dropout).
The backward is an exact function of (q, k, v, out_in, dout, lse_in):  p = exp(s - lse_in) on valid keys,  D[i] = dout[i] . out_in[i],
dP = dout v^T,  dS = p (f dP - D),  dV = (p f)^T dout,  dK = scale dS^T q,  dQ = scale dS k,  drel[b][h] = sum of dS[h] over the
(i, j) with rel_bucket[j - i + Tq - 1] == b.  So a backward kernel can be handed the rounded reference out / lse and is then judged
on its own.

The kernels' rounding points (csrc/attention.hip, attention_pair.hip, attention_long.hip) and what each costs.  u is the unit
roundoff of the 16-bit type (2^-8 bf16, 2^-11 fp16), e = 2^-24 that of fp32, A = gemm_ref.ACT_EPS = 2^-16 the project's margin for a
fast fp32 approximation (here the hardware exp2 and __logf).
  (a) The raw logit and dP are fp32 sums of 64 exact products; scale, bias and the reference value (the row's running maximum m in the
      forward, lse_in in the backward) are applied with one or two fp32 operations.  The exponent is therefore off by at most
          ds[i][j] = 2 e (66 scale |q[i]|.|k[j]| + 2 |bias| + |s| + R[i]),
      R[i] = max_valid |s[i][.]| + DEFER ln 2 in the forward (m lies between the row's maximum and DEFER log2 units above what the row
      has seen), R[i] = 2 |lse_in[i]| in the backward.
  (b) exp2 is the hardware approximation: relative error <= A.  With (a) the fp32 probability is p (1 + t), |t| <= rho = A + ds.
  (c) The forward's row sum l is taken from the unrounded fp32 probabilities in fp32: relative error <= sum_j p rho + Tk e.
  (d) P f (forward and backward) and dS are rounded to the 16-bit type before their MFMAs: relative error u.  The deferred maximum
      keeps P <= 2^DEFER, far inside both types' range.  fp16 only: P is NOT normalised, so an entry below 2^-14 rounds with an
      absolute error of up to 2^-25; the reference maximum may sit DEFER log2 units above the row's true maximum, so l >= 2^-DEFER
      and after the division by l that is an absolute 2^(DEFER - 25) per valid key: the term ETA_P * sum_j f |v[j]|.
  (e) P V, P^T dO, dS^T Q, dS K accumulate in fp32 over n = Tk (or Tq) terms in any order (blocks, chunks, the odd tile's partials):
      acc(n, T) = 2 (n + 4) e T with T the sum of the absolute terms -- the form of gemm_ref, the + 4 and the factor 2 covering the
      fp32 scale, the correctly rounded 1 / l and the few other fp32 operations.
  (f) D is an fp32 sum of 64 products: error <= 66 e |dout[i]|.|out_in[i]|.
  (g) The stored result is rounded to 16 bits: u |result|.  lse and drel stay fp32.
First-order sums of these, with ONE safety factor C = 2 on the 16-bit terms (d) and (g), which dominate every bound.  Why on both:
the worst case of the two roundings is sharp for a sum of one term (a key that a single query sees under the causal mask, Tq = 1,
the only key a dropout row keeps): both at their maximum u with the same sign give 2 u |x| and nothing averages.  With C on both
terms correct arithmetic sits at no more than half its bound on ANY data (tests/test_attention_ref.py measures it with the
emulator), so a different but legitimate summation order has room; with C on (d) alone that case would reach 2 / 3.
    out : C u |o| + (1 + u) [ C u Pv + sum_j p f |v| rho + |o| sum_j p rho + acc(Tk, Pv + |o|) + ETA_P sum_valid f |v| ],  Pv = sum_j p f |v|
    lse : acc(Tk, 1) + 4 e (R + |lse|) + max_valid ds + A (2 + n_resc + ln Tk + DEFER ln 2): lse = m ln 2 + log l; the fp32 sum l (c),
          the product m ln 2 and the last addition, the largest logit error of the row, and one absolute margin for the
          approximations of exp2 (on l), of __logf (relative A on |log l| <= ln Tk + DEFER ln 2) and of the n_resc <= (max s - min s) /
          (DEFER ln 2) rescales after a row's first block (exp2(m_old - m_new) multiplies l and the running output alike, so it
          cancels in out but not in lse)
    ddS[i][j] = |dS| rho + p [ 66 e (f |dout[i]|.|v[j]| + |dout[i]|.|out_in[i]|) + 2 e (f |dP| + |D|) ]      (the fp32 dS)
    dv  : C u |dv| + (1 + u) [ C u Pd + sum_i p f |dout| rho + acc(Tq, Pd) ],  Pd = sum_i p f |dout|
    dk  : C u |dk| + (1 + u) scale [ sum_i (C u |dS| + ddS) |q[i]| + acc(Tq, sum_i |dS| |q[i]|) ]
    dq  : the same over the keys with |k[j]|
    drel: sum of ddS over the bucket's elements + 2 (2 (Tq + Tk) + 4) e sum |dS|: the kernel sums the unrounded fp32 dS along a
          diagonal (<= min(Tq, Tk) terms), the diagonals of a bucket (<= Tq + Tk - 1), then one float atomic per workgroup (the
          caller adds the items' bounds and the fp32 error of adding the items).
Masked entries are exact zeros in every sum, so dK / dV rows of masked keys have bound 0: any non-zero value there is outside.

The emulator (emulate_forward / emulate_backward) is the same operation in fp32 torch with exactly the rounding points (a) - (g); its
`defer` in [0, 1) puts the reference maximum defer * DEFER log2 units above the row's maximum.  It shows that correct arithmetic
fits the bound and carries the mutations; a kernel is never compared with it.
"""
import math
from dataclasses import dataclass

import torch

from gemm_ref import ACT_EPS, EPS32, U_OUT, check, violations  # noqa: F401  (check / violations: re-exported for the tests)

D = 64
DEFER = 8.0                      # ATT_DEFER of csrc/attention.h, log2 units
C_SAFETY = 2.0
ETA_P = {torch.bfloat16: 0.0, torch.float16: 2.0 ** (DEFER - 25)}
LN2 = math.log(2.0)
LOG2E = 1.0 / LN2


# ------------------------------------------------------------------------------------------------------------------- operands
def valid_mask(Tq, Tk, key_len=None, causal=False, device="cpu"):
    """[Tq][Tk] bool: key j is valid for query i"""
    i = torch.arange(Tq, device=device)[:, None]
    j = torch.arange(Tk, device=device)[None, :]
    m = (j < (Tk if key_len is None else min(int(key_len), Tk))).expand(Tq, Tk)
    if causal:
        m = m & (j <= i)
    return m.clone()


def rel_bias(rel_emb, rel_bucket, Tq, Tk):
    """[H][Tq][Tk] of rel_emb[rel_bucket[j - i + Tq - 1]][h] (rel_emb [buckets][H], rel_bucket [Tq + Tk - 1])"""
    i = torch.arange(Tq, device=rel_emb.device)[:, None]
    j = torch.arange(Tk, device=rel_emb.device)[None, :]
    return rel_emb[rel_bucket.long()[j - i + Tq - 1]].permute(2, 0, 1)


def _hd(x):
    return x.double().permute(1, 0, 2)          # [T][H][64] -> [H][T][64]


def _acc(n, t):
    return 2.0 * (n + 4) * EPS32 * t


# ------------------------------------------------------------------------------------------------------------------ reference
def forward_reference(q, k, v, *, scale, dtype, valid, bias=None, drop=None):
    """-> ({"out": (ref [Tq][H][64], bound), "lse": (ref [H][Tq], bound)}, p [H][Tq][Tk]), float64.  valid [Tq][Tk] or [H][Tq][Tk]
    bool, bias / drop [H][Tq][Tk] or None.  Every row needs a valid key."""
    Q, K, V = _hd(q), _hd(k), _hd(v)
    H, Tq, Tk = Q.shape[0], Q.shape[1], K.shape[1]
    u = U_OUT[dtype]
    valid = valid.expand(H, Tq, Tk)
    b = torch.zeros((), dtype=torch.float64, device=Q.device) if bias is None else bias.double()
    f = torch.ones((), dtype=torch.float64, device=Q.device) if drop is None else drop.double()
    s = scale * (Q @ K.transpose(1, 2)) + b
    ts = abs(scale) * (Q.abs() @ K.abs().transpose(1, 2))
    sm = s.masked_fill(~valid, -math.inf)
    lse = torch.logsumexp(sm, -1)
    p = torch.exp(sm - lse[..., None])
    absmax = s.abs().masked_fill(~valid, 0.0).amax(-1)
    R = absmax + DEFER * LN2
    ds = 2.0 * EPS32 * (66.0 * ts + 2.0 * b.abs() + s.abs() + R[..., None])
    rho = ACT_EPS + ds
    pf = p * f
    o = pf @ V
    Pv = pf @ V.abs()
    fv = (valid.double() * f) @ V.abs()
    bound_o = C_SAFETY * u * o.abs() + (1 + u) * (C_SAFETY * u * Pv + (pf * rho) @ V.abs() + o.abs() * (p * rho).sum(-1, keepdim=True)
                                       + _acc(Tk, Pv + o.abs()) + ETA_P[dtype] * fv)
    smin = s.masked_fill(~valid, math.inf).amin(-1)
    n_resc = (sm.amax(-1) - smin) / (DEFER * LN2)
    bound_l = (_acc(Tk, 1.0) + 4.0 * EPS32 * (R + lse.abs()) + ds.masked_fill(~valid, 0.0).amax(-1)
               + ACT_EPS * (2.0 + n_resc + math.log(Tk) + DEFER * LN2))
    return {"out": (o.permute(1, 0, 2), bound_o.permute(1, 0, 2)), "lse": (lse, bound_l)}, p


def backward_reference(q, k, v, out_in, dout, lse_in, *, scale, dtype, valid, bias=None, drop=None, rel_bucket=None, nbuckets=0):
    """-> {"dq", "dk", "dv": (ref [T][H][64], bound)} and, with rel_bucket, "drel": (ref [buckets][H], bound) and "drel_mag"
    (sum |dS| per bucket and head, for the fp32 error of adding items), float64"""
    Q, K, V, O, dO = _hd(q), _hd(k), _hd(v), _hd(out_in), _hd(dout)
    H, Tq, Tk = Q.shape[0], Q.shape[1], K.shape[1]
    u = U_OUT[dtype]
    valid = valid.expand(H, Tq, Tk)
    b = torch.zeros((), dtype=torch.float64, device=Q.device) if bias is None else bias.double()
    f = torch.ones((), dtype=torch.float64, device=Q.device) if drop is None else drop.double()
    lse = lse_in.double()
    s = scale * (Q @ K.transpose(1, 2)) + b
    ts = abs(scale) * (Q.abs() @ K.abs().transpose(1, 2))
    p = torch.exp(s - lse[..., None]).masked_fill(~valid, 0.0)
    ds = 2.0 * EPS32 * (66.0 * ts + 2.0 * b.abs() + s.abs() + 2.0 * lse.abs()[..., None])
    rho = ACT_EPS + ds
    Dq = (dO * O).sum(-1)
    TD = (dO.abs() * O.abs()).sum(-1)
    dP = dO @ V.transpose(1, 2)
    TdP = dO.abs() @ V.abs().transpose(1, 2)
    dS = p * (f * dP - Dq[..., None])
    ddS = dS.abs() * rho + p * (66.0 * EPS32 * (f * TdP + TD[..., None]) + 2.0 * EPS32 * (f * dP.abs() + Dq.abs()[..., None]))
    pf = p * f
    dv = pf.transpose(1, 2) @ dO
    Pd = pf.transpose(1, 2) @ dO.abs()
    bound_dv = C_SAFETY * u * dv.abs() + (1 + u) * (C_SAFETY * u * Pd + (pf * rho).transpose(1, 2) @ dO.abs() + _acc(Tq, Pd))
    e16 = C_SAFETY * u * dS.abs() + ddS
    dk = scale * (dS.transpose(1, 2) @ Q)
    bound_dk = C_SAFETY * u * dk.abs() + (1 + u) * abs(scale) * (e16.transpose(1, 2) @ Q.abs() + _acc(Tq, dS.abs().transpose(1, 2) @ Q.abs()))
    dq = scale * (dS @ K)
    bound_dq = C_SAFETY * u * dq.abs() + (1 + u) * abs(scale) * (e16 @ K.abs() + _acc(Tk, dS.abs() @ K.abs()))
    out = {"dq": (dq.permute(1, 0, 2), bound_dq.permute(1, 0, 2)), "dk": (dk.permute(1, 0, 2), bound_dk.permute(1, 0, 2)),
           "dv": (dv.permute(1, 0, 2), bound_dv.permute(1, 0, 2))}
    if rel_bucket is not None:
        i = torch.arange(Tq, device=Q.device)[:, None]
        j = torch.arange(Tk, device=Q.device)[None, :]
        idx = rel_bucket.long()[j - i + Tq - 1].flatten()

        def per_bucket(x):
            return torch.zeros(nbuckets, H, dtype=torch.float64, device=Q.device).index_add_(0, idx, x.reshape(H, -1).t().contiguous())

        mag = per_bucket(dS.abs())
        out["drel"] = (per_bucket(dS), per_bucket(ddS) + 2.0 * (2 * (Tq + Tk) + 4) * EPS32 * mag)
        out["drel_mag"] = mag
    return out


def backward_dout_sensitivity(q, k, v, out_in, lse_in, b, *, scale, valid):
    """The backward is linear in dout.  For a dout known only to within b >= 0 element-wise ([Tq][H][64]; an intermediate that was
    rebuilt by its own reference), the most dq / dk / dv can move: the backward's operator with every coefficient replaced by its
    absolute value, applied to b -- dP <= b |v|^T, D <= b . |out_in|, dS <= p (dP + D), dV <= p^T b, dK <= scale dS^T |q|,
    dQ <= scale dS |k|, each times (1 + u) for the 16-bit store.  -> {"dq", "dk", "dv"} [T][H][64], float64"""
    Q, K, V, O, B = _hd(q), _hd(k), _hd(v), _hd(out_in), _hd(b)
    H, Tq, Tk = Q.shape[0], Q.shape[1], K.shape[1]
    valid = valid.expand(H, Tq, Tk)
    s = scale * (Q @ K.transpose(1, 2))
    p = torch.exp(s - lse_in.double()[..., None]).masked_fill(~valid, 0.0)
    dS = p * (B @ V.abs().transpose(1, 2) + (B * O.abs()).sum(-1)[..., None])
    up = 1 + U_OUT[torch.bfloat16]
    return {"dq": (up * abs(scale) * (dS @ K.abs())).permute(1, 0, 2), "dk": (up * abs(scale) * (dS.transpose(1, 2) @ Q.abs())).permute(1, 0, 2),
            "dv": (up * (p.transpose(1, 2) @ B)).permute(1, 0, 2)}


def worst(got, ref, bound):
    """largest |got - ref| / bound (elements with bound 0 count as 0 when exact, inf otherwise; NaN counts as inf)"""
    d = (got.double() - ref).abs()
    r = torch.where(d <= bound, d / bound.clamp_min(1e-300), torch.full_like(d, math.inf))
    r = torch.where(d == 0, torch.zeros_like(r), r)
    return float(r.max()) if r.numel() else 0.0


def compare(got, ref, bound, dtype=None):
    """None when `got` is a result the bound accepts, otherwise the reason as text: wrong shape, wrong dtype, NaN / Inf, or
    elements outside the bound"""
    if tuple(got.shape) != tuple(ref.shape):
        return f"shape {tuple(got.shape)} instead of {tuple(ref.shape)}"
    if dtype is not None and got.dtype != dtype:
        return f"dtype {got.dtype} instead of {dtype}"
    if not bool(torch.isfinite(got.double()).all()):
        return f"{int((~torch.isfinite(got.double())).sum())} non-finite elements"
    bad = violations(got, ref, bound)
    if bool(bad.any()):
        return f"{int(bad.sum())} of {bad.numel()} elements outside the bound, worst ratio {worst(got, ref, bound):.3g}"
    return None


# ------------------------------------------------------------------------------------------------------------------- emulator
def _hf(x):
    return x.float().permute(1, 0, 2)


def emulate_forward(q, k, v, *, scale, dtype, valid, bias=None, drop=None, defer=0.0, lse_dropped=None):
    """fp32 with the kernels' rounding points -> out [Tq][H][64] (dtype), lse [H][Tq] fp32.  lse_dropped: bool [H][Tq], rows whose
    row sum is (wrongly) taken from the probabilities after dropout (a mutation)."""
    Q, K, V = _hf(q), _hf(k), _hf(v)
    H, Tq, Tk = Q.shape[0], Q.shape[1], K.shape[1]
    valid = valid.expand(H, Tq, Tk)
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    s2 = (Q @ K.transpose(1, 2)) * sl2
    if bias is not None:
        s2 = s2 + bias.float() * torch.tensor(LOG2E, dtype=torch.float32)
    s2 = s2.masked_fill(~valid, -1e30)
    m = s2.amax(-1) + torch.tensor(defer * DEFER, dtype=torch.float32)
    pt = torch.exp2(s2 - m[..., None]).masked_fill(~valid, 0.0)
    pd = pt if drop is None else pt * drop.float()
    l = pt.sum(-1)
    if lse_dropped is not None:
        l = torch.where(lse_dropped, pd.sum(-1), l)
    o = (pd.to(dtype).float() @ V) * (1.0 / l)[..., None]
    lse = m * torch.tensor(LN2, dtype=torch.float32) + torch.log(l)
    return o.to(dtype).permute(1, 0, 2).contiguous(), lse


def emulate_backward(q, k, v, out_in, dout, lse_in, *, scale, dtype, valid, bias=None, drop=None, rel_bucket=None, nbuckets=0,
                     d_cols=None, dk_scale=None, kv_skip=None):
    """fp32 with the kernels' rounding points -> dq, dk, dv (dtype, [T][H][64]), drel fp32 [buckets][H] or None.  Mutation hooks:
    d_cols bool [H][Tq] (rows whose D is taken over 56 columns), dk_scale [H][Tk] (extra factor on dK), kv_skip bool [H][Tq][Tk]
    (elements left out of dK / dV only)."""
    Q, K, V, O, dO = _hf(q), _hf(k), _hf(v), _hf(out_in), _hf(dout)
    H, Tq, Tk = Q.shape[0], Q.shape[1], K.shape[1]
    valid = valid.expand(H, Tq, Tk)
    sl2 = torch.tensor(scale * LOG2E, dtype=torch.float32)
    s2 = (Q @ K.transpose(1, 2)) * sl2
    if bias is not None:
        s2 = s2 + bias.float() * torch.tensor(LOG2E, dtype=torch.float32)
    lse2 = lse_in.float() * torch.tensor(LOG2E, dtype=torch.float32)
    p = torch.exp2(s2 - lse2[..., None]).masked_fill(~valid, 0.0)
    Dq = (dO * O).sum(-1)
    if d_cols is not None:
        Dq = torch.where(d_cols, (dO[..., :56] * O[..., :56]).sum(-1), Dq)
    dP = dO @ V.transpose(1, 2)
    f = None if drop is None else drop.float()
    dS = p * ((dP if f is None else dP * f) - Dq[..., None])
    pf = p if f is None else p * f
    p16, dS16 = pf.to(dtype).float(), dS.to(dtype).float()
    if kv_skip is not None:
        p16k, dS16k = p16.masked_fill(kv_skip, 0.0), dS16.masked_fill(kv_skip, 0.0)
    else:
        p16k, dS16k = p16, dS16
    sc = torch.tensor(scale, dtype=torch.float32)
    dv = p16k.transpose(1, 2) @ dO
    dk = (dS16k.transpose(1, 2) @ Q) * sc
    if dk_scale is not None:
        dk = dk * dk_scale.float()[..., None]
    dq = (dS16 @ K) * sc
    drel = None
    if rel_bucket is not None:
        i = torch.arange(Tq, device=Q.device)[:, None]
        j = torch.arange(Tk, device=Q.device)[None, :]
        idx = rel_bucket.long()[j - i + Tq - 1].flatten()
        drel = torch.zeros(nbuckets, H, dtype=torch.float32, device=Q.device).index_add_(0, idx, dS.reshape(H, -1).t().contiguous())
    r = lambda x: x.to(dtype).permute(1, 0, 2).contiguous()          # noqa: E731
    return r(dq), r(dk), r(dv), drel


# ---------------------------------------------------------------------------------------------------------------------- items
@dataclass
class Item:
    """one item of a case: the logical operands and everything a mutation needs"""
    q: torch.Tensor               # [Tq][H][64], 16-bit
    k: torch.Tensor               # [Tk][H][64]
    v: torch.Tensor
    dout: torch.Tensor            # [Tq][H][64]
    scale: float
    dtype: torch.dtype
    key_len: object = None        # valid keys (None: Tk)
    causal: bool = False
    rel_emb: object = None        # [buckets][H] fp32
    rel_bucket: object = None     # [Tq + Tk - 1] int
    drop: object = None           # [H][Tq][Tk] dropout factors
    drop_dense: object = None     # flat factors of the dense call this item belongs to, from element (item, head 0, query 0, key 0)
    dense_tq: int = 0             # that call's tq / tk (the dropout coordinates); 0: the item's own
    dense_tk: int = 0
    behind_k: object = None       # [H][64] the K / V rows right behind the item's last key (the dense twin's padding rows of a packed
    behind_v: object = None       #   item); None: the zero padding the kernels stage behind Tk

    @property
    def Tq(self):
        return self.q.shape[0]

    @property
    def Tk(self):
        return self.k.shape[0]

    @property
    def H(self):
        return self.q.shape[1]

    @property
    def kvalid(self):
        return self.Tk if self.key_len is None else min(int(self.key_len), self.Tk)

    def valid(self):
        return valid_mask(self.Tq, self.Tk, self.key_len, self.causal, self.q.device)

    def bias(self):
        return None if self.rel_emb is None else rel_bias(self.rel_emb, self.rel_bucket, self.Tq, self.Tk)

    def nbuckets(self):
        return 0 if self.rel_emb is None else self.rel_emb.shape[0]

    def fwd_ref(self):
        return forward_reference(self.q, self.k, self.v, scale=self.scale, dtype=self.dtype, valid=self.valid(), bias=self.bias(),
                                 drop=self.drop)

    def bwd_ref(self, out_in, lse_in):
        return backward_reference(self.q, self.k, self.v, out_in, self.dout, lse_in, scale=self.scale, dtype=self.dtype,
                                  valid=self.valid(), bias=self.bias(), drop=self.drop, rel_bucket=self.rel_bucket,
                                  nbuckets=self.nbuckets())

    def emulate(self, out_in, lse_in, defer=0.0, with_bwd=True):
        """the correct arithmetic: dict of the outputs (the backward on out_in / lse_in)"""
        o, l = emulate_forward(self.q, self.k, self.v, scale=self.scale, dtype=self.dtype, valid=self.valid(), bias=self.bias(),
                               drop=self.drop, defer=defer)
        res = {"out": o, "lse": l}
        if with_bwd:
            dq, dk, dv, drel = emulate_backward(self.q, self.k, self.v, out_in, self.dout, lse_in, scale=self.scale, dtype=self.dtype,
                                                valid=self.valid(), bias=self.bias(), drop=self.drop, rel_bucket=self.rel_bucket,
                                                nbuckets=self.nbuckets())
            res.update(dq=dq, dk=dk, dv=dv)
            if drel is not None:
                res["drel"] = drel
        return res


# ------------------------------------------------------------------------------------------------------------------ mutations
MUTATIONS = ("admit_first_masked", "drop_last_valid", "causal_plus_one", "causal_minus_one", "swap_rows", "row_unwritten",
             "head_shift", "dk_scale_missing", "dk_scale_twice", "drop_packed_coords", "drop_shift_key", "bias_diag_off",
             "lse_without_drop_correction", "d_56_columns", "masked_key_nonzero", "skip_chunk")


def _tile(tile, T):
    return slice(16 * tile, min(16 * tile + 16, T))


def mutate(it, name, out_in, lse_in, head=0, tile=0, with_bwd=True):
    """the outputs of a kernel that is wrong in ONE way, for head `head` and the 16-row tile `tile` only (queries for the forward
    and dQ, keys for the dK / dV mutations), through the emulator's rounding -> dict like Item.emulate, or None when the mutation
    does not apply to this item (nothing would change)"""
    H, Tq, Tk = it.H, it.Tq, it.Tk
    dev = it.q.device
    valid = it.valid().expand(H, Tq, Tk).clone()
    bias, drop = it.bias(), None if it.drop is None else it.drop.clone()
    k, v = it.k, it.v
    rs, ks = _tile(tile, Tq), _tile(tile, Tk)
    rows = torch.arange(Tq, device=dev)[rs]
    if rows.numel() == 0:
        return None
    kv = it.kvalid
    fkw, bkw, post = {}, {}, None
    ext = False
    if name == "admit_first_masked":
        if kv < Tk:
            valid[head, rs, kv] = True
        else:                       # the row behind the item: the dense twin's, or the staged zero padding
            if it.behind_k is None and all(int(r) in getattr(it, "stressed", ()) for r in rows):
                return None         # a zero key with a zero value moves a row by exp(-lse): only a row without a dominant key shows it
            bk = torch.zeros(H, D, dtype=it.dtype, device=dev) if it.behind_k is None else it.behind_k
            bv = torch.zeros(H, D, dtype=it.dtype, device=dev) if it.behind_v is None else it.behind_v
            k, v = torch.cat([k, bk[None]]), torch.cat([v, bv[None]])
            valid = torch.cat([valid, torch.zeros(H, Tq, 1, dtype=torch.bool, device=dev)], -1)
            valid[head, rs, Tk] = True
            if bias is not None:
                bias = torch.cat([bias, torch.zeros(H, Tq, 1, dtype=bias.dtype, device=dev)], -1)
            if drop is not None:
                drop = torch.cat([drop, torch.ones(H, Tq, 1, dtype=drop.dtype, device=dev)], -1)
            ext = True
    elif name == "drop_last_valid":
        last = torch.clamp(rows, max=kv - 1) if it.causal else torch.full_like(rows, kv - 1)
        sel = last >= 1                 # a row keeps at least one key
        if not bool(sel.any()):
            return None
        valid[head, rows[sel], last[sel]] = False
    elif name == "causal_plus_one":
        sel = rows + 1 < kv
        if not it.causal or not bool(sel.any()):
            return None
        valid[head, rows[sel], rows[sel] + 1] = True
    elif name == "causal_minus_one":
        sel = (rows >= 1) & (rows < kv)
        if not it.causal or not bool(sel.any()):
            return None
        valid[head, rows[sel], rows[sel]] = False
    elif name == "swap_rows":
        a = int(rows[0])
        other = [int(r) for r in rows[1:] if not torch.equal(it.q[int(r)], it.q[a])]          # (stressed rows share their query)
        if not other:
            return None
        b = other[0]

        def post(res):
            for key in ("out", "dq"):
                if key in res:
                    res[key][[a, b], head] = res[key][[b, a], head]
            res["lse"][head, [a, b]] = res["lse"][head, [b, a]]
    elif name == "row_unwritten":
        def post(res):
            a = int(rows[-1])
            for key in ("out", "dq"):
                if key in res:
                    res[key][a, head] = 0
    elif name == "head_shift":
        if head + 1 >= H:
            return None

        def post(res):
            for key in ("out", "dq"):
                if key in res:
                    res[key][rs, head + 1] = res[key][rs, head]
    elif name in ("dk_scale_missing", "dk_scale_twice"):
        if it.scale == 1.0 or not with_bwd or kv == 1:          # (one valid key: p = 1, dS = 0 and dK = 0 exactly)
            return None
        sc = torch.ones(H, Tk, device=dev)
        sc[head, ks] = 1.0 / it.scale if name == "dk_scale_missing" else it.scale
        bkw["dk_scale"] = sc
    elif name == "drop_packed_coords":
        if drop is None or it.drop_dense is None or (it.dense_tq in (0, Tq) and it.dense_tk in (0, Tk)):
            return None
        idx = ((head * Tq + rows)[:, None] * Tk + torch.arange(Tk, device=dev)[None, :])
        drop[head, rs] = it.drop_dense[idx]
        if torch.equal((drop * valid)[head, rs], (it.drop * valid)[head, rs]):
            return None
    elif name == "drop_shift_key":
        if drop is None or Tk < 2:
            return None
        drop[head, rs] = torch.roll(drop[head, rs], 1, -1)
        if torch.equal((drop * valid)[head, rs], (it.drop * valid)[head, rs]):
            return None
    elif name == "bias_diag_off":
        if bias is None:
            return None
        i = rows[:, None]
        j = torch.arange(Tk, device=dev)[None, :]
        bias = bias.clone()
        bias[head, rs] = it.rel_emb[it.rel_bucket.long()[(j - i + Tq).clamp(0, Tq + Tk - 2)], head]
    elif name == "lse_without_drop_correction":
        if drop is None:
            return None
        sel = torch.zeros(H, Tq, dtype=torch.bool, device=dev)
        sel[head, rs] = True
        fkw["lse_dropped"] = sel
    elif name == "d_56_columns":
        if not with_bwd:
            return None
        sel = torch.zeros(H, Tq, dtype=torch.bool, device=dev)
        sel[head, rs] = True
        bkw["d_cols"] = sel
    elif name == "masked_key_nonzero":
        if kv >= Tk or not with_bwd:
            return None

        def post(res):
            res["dk"][kv, head, 0] = 2.0 ** -20
            res["dv"][Tk - 1, head, D - 1] = -2.0 ** -20
    elif name == "skip_chunk":
        if Tk <= 128:
            return None
        c0 = 128 * ((Tk - 1) // 128) if Tk <= 256 else 128          # the last (partial) chunk, or the second of several
        valid_f = valid.clone()
        valid_f[head, rs, c0:c0 + 128] = False
        skip = torch.zeros(H, Tq, Tk, dtype=torch.bool, device=dev)
        if Tq > 64:
            skip[head, 64:128, ks] = True
        bkw["kv_skip"] = skip
        if torch.equal(valid_f, valid) and not (with_bwd and bool((skip & valid).any())):
            return None
    else:
        raise ValueError(name)
    vf = valid_f if name == "skip_chunk" else valid
    o, l = emulate_forward(it.q, k, v, scale=it.scale, dtype=it.dtype, valid=vf, bias=bias, drop=drop, **fkw)
    res = {"out": o, "lse": l}
    if with_bwd:
        vb = it.valid().expand(H, Tq, Tk) if name == "skip_chunk" else valid
        dq, dk, dv, drel = emulate_backward(it.q, k, v, out_in, it.dout, lse_in, scale=it.scale, dtype=it.dtype, valid=vb, bias=bias,
                                            drop=drop, rel_bucket=None if ext else it.rel_bucket, nbuckets=it.nbuckets(), **bkw)
        if ext:
            dk, dv = dk[:Tk].contiguous(), dv[:Tk].contiguous()
            drel = None
        res.update(dq=dq, dk=dk, dv=dv)
        if drel is not None:
            res["drel"] = drel
    if post is not None:
        post(res)
    return res


# --------------------------------------------------------------------------------------------------- inputs that stress the mask edge
def stress_rows(Tq, klens):
    """the query rows that point at the last valid key: the first and the last row and the rows on both sides of every 16-row tile
    boundary that a mask edge (one of `klens`, or Tq itself) touches"""
    rows = {0, Tq - 1}
    for e in set(klens) | {Tq}:
        b = (int(e) // 16) * 16
        for r in (b - 1, b, b + 15, b + 16, int(e) - 1, int(e)):
            if 0 <= r < Tq:
                rows.add(r)
    return sorted(rows)


def _operands(Tq, Tk, H, dtype, gen, *, key_len=None, causal=False, own_q=None, own_k=None, device="cpu"):
    """q [Tq][H][64], k, v [Tk][H][64], dout [Tq][H][64] (16-bit) for one item.  own_q / own_k: the item's packed query / key count
    inside a dense twin of Tq / Tk rows (rows behind it are padding: they hold finite values that would dominate if they were read).
    Ordinary rows are randn.  With a unit vector w per head: the stressed query rows (stress_rows) are 24 w and the item's last valid
    key is 3 w, so that key holds a large share of their probability (logit 9 against N(0, 9) of the others); every masked key
    (>= key_len, or behind own_len) is 4 w with value rows of standard deviation 8 (logit 12: it would take over the row); under a
    causal mask the key behind each stressed row's diagonal is 4 w with such a value row as well.  A few other rows (spike rows) are
    24 w2 with a second unit vector w2; one early key is 6 w2 and one late key 9 w2 (logits 18 and 27 there): the late one lies 9
    above whatever the row has seen and forces the rescale of the deferred maximum, the early one leaves every later block far below
    the reference.  Finite values only.  -> q, k, v, dout, the stressed rows"""
    rn = lambda *s: torch.randn(*s, generator=gen, device=device)          # noqa: E731
    q, k, v, do = rn(Tq, H, D), rn(Tk, H, D), rn(Tk, H, D), rn(Tq, H, D)
    w = rn(H, D)
    w = w / w.norm(dim=-1, keepdim=True)
    n_q = Tq if own_q is None else own_q
    n_k = Tk if own_k is None else own_k
    kv = n_k if key_len is None else min(int(key_len), n_k)
    srows = [r for r in stress_rows(n_q, [kv]) if r < n_q]
    q[srows] = 24.0 * w
    k[kv - 1] = 3.0 * w
    spikes = set()
    if kv >= 8:
        w2 = rn(H, D)
        w2 = w2 / w2.norm(dim=-1, keepdim=True)
        late = [j for j in range(kv - 3, kv - 8, -1) if j not in srows and not (causal and j - 1 in srows)][0]
        spikes = {1, late}
        k[1], k[late] = 6.0 * w2, 9.0 * w2
        for r in (2, n_q // 2, n_q - 3):
            if 0 <= r < n_q and r not in srows:
                q[r] = 24.0 * w2
    if causal:
        for r in srows:
            if r < kv and r not in spikes:
                k[r] = 3.0 * w
            if r + 1 < kv and (r + 1) not in srows and (r + 1) not in spikes:
                k[r + 1] = 4.0 * w
                v[r + 1] = 8.0 * rn(H, D)
    if kv < Tk:
        k[kv:] = 4.0 * w
        v[kv:] = 8.0 * rn(Tk - kv, H, D)
    if n_q < Tq:
        q[n_q:] = 24.0 * w
        do[n_q:] = 0.0          # as in the models: the padded call equals the packed one only when no gradient enters at a padding row
    return q.to(dtype), k.to(dtype), v.to(dtype), do.to(dtype), srows


def default_buckets(Tq, Tk, nbuckets, device="cpu"):
    """a bucket per key - query offset: exact near the diagonal, coarser further out (every bucket in use when the range allows)"""
    d = torch.arange(Tq + Tk - 1, device=device) - (Tq - 1)
    half = nbuckets // 2
    mag = d.abs()
    b = torch.where(mag < half // 2, mag, (half // 2 + torch.log2((mag.float() + 1) / (half // 2 + 1)).floor().long()).clamp(max=half - 1))
    return (b + half * (d > 0)).int()


# ---------------------------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    """one call of the C ABI.  api: "qkv" (uniir_attention_fwd / _bwd), "f16" (uniir_attention_fwd_f16, forward only), "packed"
    (_fwd_packed / _bwd_packed, lens = the items' lengths), "ex" (_fwd_ex / _bwd_ex), "rows" (_fwd_rows / _bwd_rows, lens = the
    items' query lengths), "rel" (uniir_attention_rel_fwd / _bwd)."""
    name: str
    path: str                     # the kernel instantiations the case is meant to reach
    api: str
    batch: int
    heads: int
    tq: int
    tk: int = 0                   # 0: tq
    causal: bool = False
    key_len: object = None        # per item, or None
    lens: object = None           # per item ("packed", "rows")
    kv_packed: int = 0            # "rows"
    drop_p: float = 0.0
    nbuckets: int = 0             # "rel"
    dtype: torch.dtype = torch.bfloat16
    bwd: bool = True
    chained: bool = False         # once more on the kernel's own forward results
    pad: int = 0                  # extra elements on every leading dimension the entry point lets the caller choose
    seed: int = 0

    def __post_init__(self):
        self.tk = self.tk or self.tq
        if self.api == "f16":
            self.dtype, self.bwd = torch.float16, False


def build_items(c, device, dropf=None):
    """the items of a case -> list of Item.  Every item also carries `twin`: its (q, k, v, dout) of the full tq / tk rows (what the
    dense padded call of a packed case reads; the item's own operands are their leading rows) and `twin_key_len`.  dropf(count) ->
    count dropout factors (fp32, flat) of the call's dense coordinates; needed when c.drop_p > 0."""
    gen = torch.Generator(device=device).manual_seed(1000 + c.seed)
    H = c.heads
    scale = 1.0 if c.api == "rel" else 0.125
    drop_all = None
    if c.drop_p > 0:
        drop_all = dropf(c.batch * H * c.tq * c.tk).reshape(c.batch, H, c.tq, c.tk)
    emb = bucket = None
    if c.api == "rel":
        emb = torch.randn(c.nbuckets, H, generator=gen, device=device)
        bucket = default_buckets(c.tq, c.tk, c.nbuckets, device)
    items = []
    for m in range(c.batch):
        own_q = own_k = None
        klen = None if c.key_len is None else int(c.key_len[m])
        if c.lens is not None:
            own_q = int(c.lens[m])
            own_k = own_q if (c.api == "packed" or c.kv_packed) else None
        q, k, v, do, srows = _operands(c.tq, c.tk, H, c.dtype, gen, key_len=klen, causal=c.causal, own_q=own_q, own_k=own_k, device=device)
        if scale == 1.0:
            q = (q.float() * 0.125).to(c.dtype)          # exact: T5 applies no 1 / sqrt(d), its weights are small instead
        lq = c.tq if own_q is None else own_q
        lk = c.tk if own_k is None else own_k
        it = Item(q[:lq], k[:lk], v[:lk], do[:lq], scale, c.dtype, key_len=klen, causal=c.causal, rel_emb=emb, rel_bucket=bucket,
                  drop=None if drop_all is None else drop_all[m, :, :lq, :lk],
                  drop_dense=None if drop_all is None else drop_all[m].flatten(), dense_tq=c.tq, dense_tk=c.tk,
                  behind_k=k[lk] if lk < c.tk else None, behind_v=v[lk] if lk < c.tk else None)
        it.twin = (q, k, v, do)
        it.stressed = srows
        it.twin_key_len = own_k if own_k is not None else (klen if klen is not None else c.tk)
        items.append(it)
    return items
