"""fp64 references of the fp32 kernels (norms, loss path, optimizer) and element-wise error bounds derived from their arithmetic.

Not a test module: tests/test_norm_paths_gpu.py and tests/test_loss_paths_gpu.py compare every kernel path against it, and
tests/test_fp32_ref.py checks on the CPU that a plain fp32 restatement stays inside every bound and that planted defects do not.
Every function restates one operation as include/uniir_hip.h and the kernels' comments state it, in float64, and returns
name -> (reference, bound) like gemm_ref.gemm_reference; check / violations are gemm_ref's (NaN / Inf are violations, no element is
left out).  Inputs are the logical fp32 operands (views already taken out of their strided buffers).

Constants
  EPS32 = 2^-24   unit roundoff of fp32: one rounded operation has a relative error <= EPS32.
  U_BF16 = 2^-8   unit roundoff of a round-to-nearest-even bf16 store (8 significant bits: spacing 2^-7); ETA_BF16 = 2^-134, half the smallest
                  subnormal.  A 16-bit output with fp32 error e has the bound U_BF16 * (|r| + e) + e + ETA_BF16.
  gamma(k) = k EPS32 / (1 - k EPS32): a sum whose every term passes through at most k rounded additions is within gamma(k) * sum |t|
                  of the exact sum, in any association.  One wave's sum of n terms: ceil(n / 64) per lane (a float4 adds as a two-level
                  tree), then the 6-level butterfly: wave_depth(n) = ceil(n / 64) + 6.  A 256-thread block sum of n terms:
                  ceil(n / 256) + 8.  The column sums of the norm backward (dgamma, dbeta, dx_colsum): a wave adds its rows one after
                  the other -- at most ceil(rows / 1024) of them, since at least 256 workgroups of 4 waves are resident -- the four
                  waves add as a tree (2), and the at most ceil(rows / 4) workgroup partials and the prior contents are added in
                  some order (stored partials in a fixed one, atomics in any): col_depth(rows) = ceil(rows / 1024) + ceil(rows / 4)
                  + 3.  Where every term and the prior contents are integers and their absolute sum stays below 2^24, every order
                  is exact and the bound is 0: the long cases feed integer dy, so one lost row or workgroup shows in dbeta.
  Device math functions, relative budget per call = ULP * 2 EPS32 (one ulp is at most 2 EPS32 relative).  The ROCm installation ships
  no math-accuracy table (nothing under its share / include trees states ulp figures), so the budgets are chosen here, from the
  publicly documented HIP device-function accuracies (expf 1, logf 1, rsqrtf 1, sqrtf 1 ulp, division correctly rounded = 0.5 ulp
  in the default build: no fast-math flag is passed) with a margin of 4x, respectively 4x on the 0.5 ulp of sqrt / division:
      RSQRT_ULP = 4, EXP_ULP = 4, LOG_ULP = 4, SQRT_ULP = 2, DIV_ULP = 2
  The host's powf / sqrtf of AdamW's bias corrections get POW_ULP = 2 (glibc states 1 ulp).
  MARGIN = 2      every bound returned here is twice the worst case derived below.  Round-to-nearest attains its own half ulp, so
                  a correct implementation sits at a ratio |got - ref| / bound of up to 1 of the derived figure; with the margin it
                  sits at 0.5 or less, which tests/test_fp32_ref.py asserts for an fp32 restatement of every case -- a ratio above
                  0.5 then shows a derivation that misses an operation.  A bound of 0 (exact results: hits, products with a 0 / 1
                  mask) stays 0.
  TINY32 = 2^-126 absolute term of every non-zero bound: a result in fp32's subnormal range may be flushed (an exp that underflows).

LayerNorm / RMS norm.  With d = wave_depth(width), mean |x| = m1, centred c_i = |x_i - mu|, sigma^2 = var + eps:
  e_mu  = gamma(d + 2) * m1                                  (the sum, times the rounded 1 / width)
  e_var = gamma(d + 8) * (var + e_mu^2) + e_mu^2             (a uniform shift of the mean adds exactly shift^2 to the variance; the
                                                              rest is the squares' and the sum's rounding)
  rho   = e_var / sigma^2 + (2 RSQRT_ULP + 2) EPS32          relative error of rstd (twice the first-order term: covers the second)
  |xhat^ - xhat| <= rstd * (e_mu + EPS32 c_i) (1 + rho) + |xhat_i| (rho + 2 EPS32)
so a row of large mean and small variance (|x|max / sigma large) gets the wider bound through e_mu * rstd and e_mu^2 / sigma^2: the
bound carries the row's conditioning, it is not a global constant.  y adds gamma's product and beta's addition (3 EPS32).  The
backward propagates e_xhat through g = dy gamma, c1 = mean g, c2 = mean(g xhat) and dx = rstd (g - c1 - xhat c2) (+ dres); dgamma,
dbeta and dx_colsum are prior + sum over rows, any order.  dx_f32 is unscaled; dx_bf16 and dx_colsum are scaled by branch_scale[row].

sgemm.  The product is the pinned arithmetic: one fmaf chain in ascending k per element (oracle.c_oracle.infonce_scores), bit for bit.
alpha = fl32(alpha_host * alpha_dev), applied with one fp32 multiply.  Accumulating onto C: with alpha == 1 an exact fp32 add; with
alpha != 1 either fl(c + fl(acc alpha)) or fma(acc, alpha, c), accepted element by element (sgemm_accepts).  The build contracts
floating-point expressions (hipcc's default -ffp-contract=fast and nothing in csrc/Makefile turns it off), so `*c + acc * alpha`
compiles to the fma form; the test prints how many elements matched which form.  The split-K form is per-slice chains added in
slice order with the host's splits / kslice / used arithmetic restated in splitk_plan.

InfoNCE, hard negatives, softce: the logits are an input of the statistics (the kernels read their own fp32 logits back), so lse,
loss, hit and the gradients are restated on the fp32 logits; exp's argument carries its subtraction's rounding, the sums a gamma of
their depth, log and the divisions their budgets.  The first-index arg-max is exact.
"""
import math

import numpy as np
import torch

from gemm_ref import check, violations  # noqa: F401  (re-exported: one check for every reference)

EPS32 = 2.0 ** -24
U_BF16 = 2.0 ** -8
ETA_BF16 = 2.0 ** -134
RSQRT_ULP, EXP_ULP, LOG_ULP, SQRT_ULP, DIV_ULP, POW_ULP = 4, 4, 4, 2, 2, 2
R_RSQRT, R_EXP, R_LOG, R_SQRT, R_DIV, R_POW = (2.0 * EPS32 * u for u in (RSQRT_ULP, EXP_ULP, LOG_ULP, SQRT_ULP, DIV_ULP, POW_ULP))
MARGIN = 2.0
TINY32 = 2.0 ** -126
LN_MAX_WIDTH = 2048


def _margin(fn):
    """the reference function with MARGIN and TINY32 applied to every bound it returns"""
    import functools

    @functools.wraps(fn)
    def wrapped(*a, **kw):
        out = fn(*a, **kw)
        return {k: (r, torch.where(b > 0, MARGIN * b + TINY32, torch.zeros_like(b)) if isinstance(b, torch.Tensor)
                    else (MARGIN * b + TINY32 if b > 0 else 0.0)) for k, (r, b) in out.items()}
    return wrapped


def gamma(k):
    return k * EPS32 / (1.0 - k * EPS32)


def wave_depth(n):
    return -(-n // 64) + 6


def block_depth(n):
    return -(-n // 256) + 8


def col_depth(rows):
    return -(-rows // 1024) + -(-rows // 4) + 3


def _exact_int_sum(terms, prior):
    """per column: True where every term and the prior are integers and sum |.| < 2^24 -- fp32 adds them exactly in any order"""
    ints = ((terms == terms.round()).all(0)) & (prior == prior.round())
    return ints & (terms.abs().sum(0) + prior.abs() < 2.0 ** 24)


def bf16_bound(ref, e):
    """bound of the bf16 store of a value whose fp32 form is within e of ref"""
    return U_BF16 * (ref.abs() + e) + e + ETA_BF16


def worst_ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (inf where one is NaN / Inf); 0 / 0 counts as 0"""
    d = (got.double() - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound)
    r = torch.where(torch.isfinite(got.double()) & ~torch.isnan(r), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------------------------------------------ host arithmetic
def ln_path(width):
    """(NC, EXACT) of ln_fwd_kernel / ln_bwd_kernel for a width, as csrc/norm.hip's ln_nc chooses it"""
    assert width > 0 and width % 4 == 0 and width <= LN_MAX_WIDTH
    c = (width // 4 + 63) // 64
    nc = 2 if c <= 2 else (3 if c == 3 else (4 if c == 4 else 8))
    return nc, width == 256 * nc


def sgemm_big(M, N, K, a_ck, a_cm, b_ck, b_cn, a_aligned=True, b_aligned=True, lda=4, ldb=4):
    """launch_sgemm's predicate for the 128-tile kernel (a_ck: A's k stride is 1, a_cm: its m stride is 1; likewise B)"""
    def vec_ok(aligned, ld, contig_k, ext):
        return aligned and ld % 4 == 0 and (contig_k or ext % 4 == 0)
    return (K % 16 == 0 and M >= 64 and N >= 64 and M * N >= 128 * 128 * 8 and (a_ck or a_cm) and (b_ck or b_cn)
            and vec_ok(a_aligned, lda, a_ck, M) and vec_ok(b_aligned, ldb, b_ck, N))


def sgemm_kernel_name(M, N, K, a_ck, a_cm, b_ck, b_cn, **kw):
    """S1 (sgemm_kernel) or S2..S5 = sgemm128_kernel<A_CK, B_CK> for <1,1>, <1,0>, <0,1>, <0,0>"""
    if not sgemm_big(M, N, K, a_ck, a_cm, b_ck, b_cn, **kw):
        return "S1"
    return {(True, True): "S2", (True, False): "S3", (False, True): "S4", (False, False): "S5"}[(bool(a_ck), bool(b_ck))]


def splitk_plan(M, N, K):
    """(splits, kslice, used) of uniir_sgemm_splitk: the workspace is sized by splits, the slices that run and the reduce by used"""
    tiles = -(-M // 128) * -(-N // 128)
    s = -(-1024 // tiles)
    s = max(1, min(s, K // (16 * 8)))
    ksteps = K // 16
    kslice = -(-ksteps // s) * 16
    used = -(-K // kslice)
    return s, kslice, used


def splitk_splits_form(M, N, K, a_ck, a_cm, b_ck, b_cn, a_aligned=True, b_aligned=True, lda=4, ldb=4):
    """True when uniir_sgemm_splitk takes the slab form (S6), False when it falls back to launch_sgemm"""
    def vec_ok(aligned, ld, contig_k, ext):
        return aligned and ld % 4 == 0 and (contig_k or ext % 4 == 0)
    splits = splitk_plan(M, N, K)[0]
    return not (splits < 2 or K % 16 or N % 4 or not (a_ck or a_cm) or not (b_ck or b_cn)
                or not vec_ok(a_aligned, lda, a_ck, M) or not vec_ok(b_aligned, ldb, b_ck, N))


# ----------------------------------------------------------------------------------------------------------------------- the norms
def _norm_stats(x, eps, rms):
    x = x.double()
    W = x.shape[1]
    d = wave_depth(W)
    m1 = x.abs().mean(1, keepdim=True)
    if rms:
        mu = torch.zeros_like(m1)
        e_mu = torch.zeros_like(m1)
    else:
        mu = x.mean(1, keepdim=True)
        e_mu = gamma(d + 2) * m1
    xc = x - mu
    var = (xc * xc).mean(1, keepdim=True)
    e_var = gamma(d + 8) * (var + e_mu ** 2) + e_mu ** 2
    sig2 = var + float(np.float32(eps))          # eps as the entry point receives it
    rstd = sig2.rsqrt()
    rho = e_var / sig2 + R_RSQRT + 2 * EPS32
    xhat = xc * rstd
    e_xhat = rstd * (e_mu + EPS32 * xc.abs()) * (1 + rho) + xhat.abs() * (rho + 2 * EPS32)
    return xhat, e_xhat, rstd, rho


@_margin
def norm_fwd(x, gamma_, beta, eps, rms=False):
    """x [rows][width], gamma_ / beta [width] (beta ignored in RMS mode) -> y_f32, y_bf16"""
    xhat, e_xhat, _, _ = _norm_stats(x, eps, rms)
    g = gamma_.double()[None, :]
    y = xhat * g
    if not rms:
        y = y + beta.double()[None, :]
    e = g.abs() * e_xhat + 3 * EPS32 * ((xhat * g).abs() + y.abs())
    return {"y_f32": (y, e), "y_bf16": (y, bf16_bound(y, e))}


@_margin
def norm_bwd(x, gamma_, dy, eps, rms=False, dres=None, branch_scale=None, dgamma0=None, dbeta0=None, colsum0=None):
    """dy [rows][width] fp32 or bf16 (widened exactly); dres [rows][width]; branch_scale [rows]; dgamma0 / dbeta0 / colsum0 the prior
    contents that the sums are added onto.  -> dx_f32 (unscaled), dx_bf16 (scaled by branch_scale), dgamma, dbeta (not in RMS mode),
    dx_colsum (scaled; when colsum0 is given)"""
    xhat, e_xhat, rstd, rho = _norm_stats(x, eps, rms)
    R, W = xhat.shape
    d = wave_depth(W)
    dy = dy.double()
    g = dy * gamma_.double()[None, :]
    e_g = EPS32 * g.abs()
    if rms:
        c1 = xhat.new_zeros(R, 1)
        e_c1 = torch.zeros_like(c1)
    else:
        c1 = g.mean(1, keepdim=True)
        e_c1 = (gamma(d + 2) + EPS32) * g.abs().mean(1, keepdim=True)
    gx = g * xhat
    c2 = gx.mean(1, keepdim=True)
    e_c2 = gamma(d + 4) * gx.abs().mean(1, keepdim=True) + (g.abs() * e_xhat + e_g * xhat.abs()).mean(1, keepdim=True)
    inner = g - c1 - xhat * c2
    mag = g.abs() + c1.abs() + (xhat * c2).abs()
    e_inner = e_g + e_c1 + xhat.abs() * e_c2 + c2.abs() * e_xhat + e_xhat * e_c2 + 3 * EPS32 * mag
    dx = inner * rstd
    e_dx = rstd * e_inner * (1 + rho) + (rho + EPS32) * dx.abs()
    if dres is not None:
        dx = dx + dres.double()
        e_dx = e_dx + EPS32 * dx.abs()
    out = {"dx_f32": (dx, e_dx)}
    if branch_scale is not None:
        bs = branch_scale.double()[:, None]
        sdx = dx * bs
        e_sdx = bs.abs() * e_dx + EPS32 * sdx.abs()
    else:
        sdx, e_sdx = dx, e_dx
    out["dx_bf16"] = (sdx, bf16_bound(sdx, e_sdx))
    gr = gamma(col_depth(R))
    t = dy * xhat
    dg0 = xhat.new_zeros(W) if dgamma0 is None else dgamma0.double()
    out["dgamma"] = (dg0 + t.sum(0), (dy.abs() * e_xhat + EPS32 * t.abs()).sum(0) + gr * (t.abs().sum(0) + dg0.abs()))
    if not rms:
        db0 = xhat.new_zeros(W) if dbeta0 is None else dbeta0.double()
        e_db = gr * (dy.abs().sum(0) + db0.abs())
        out["dbeta"] = (db0 + dy.sum(0), torch.where(_exact_int_sum(dy, db0), torch.zeros_like(e_db), e_db))
    if colsum0 is not None:
        cs0 = colsum0.double()
        out["dx_colsum"] = (cs0 + sdx.sum(0), e_sdx.sum(0) + gr * (sdx.abs().sum(0) + cs0.abs()))
    return out


def norm_bwd_dy_sensitivity(x, gamma_, b, eps, rms=False):
    """The norm backward is linear in dy.  For a dy known only to within b >= 0 element-wise (an intermediate that no longer exists
    and was rebuilt by its own reference), the most each result can move: the operator of norm_bwd with every coefficient replaced by
    its absolute value, applied to b.  With g = |gamma| b:  dx <= rstd (g + mean g + |xhat| mean(g |xhat|)),  dgamma <= sum_rows b |xhat|,
    dbeta <= sum_rows b,  dx_colsum <= the column sums of the dx term.  A derivation, not a measurement; it carries no margin of its
    own because b already has its reference's."""
    xhat, _, rstd, _ = _norm_stats(x, eps, rms)
    b = b.double()
    g = b * gamma_.double().abs()[None, :]
    c1 = xhat.new_zeros(xhat.shape[0], 1) if rms else g.mean(1, keepdim=True)
    dx = rstd * (g + c1 + xhat.abs() * (g * xhat.abs()).mean(1, keepdim=True))
    return {"dx_f32": dx, "dx_bf16": (1 + U_BF16) * dx, "dgamma": (b * xhat.abs()).sum(0), "dbeta": b.sum(0), "dx_colsum": dx.sum(0)}


# ------------------------------------------------------------------------------------------------------------------------- sgemm
def chain(A, B):
    """the pinned product: A [M][K], B [K][N] logical fp32 operands -> fp32 [M][N], one fmaf chain in ascending k per element"""
    from oracle import c_oracle
    A = np.ascontiguousarray(A, np.float32)
    Bt = np.ascontiguousarray(np.asarray(B, np.float32).T)
    return c_oracle.infonce_scores(A, Bt, 1.0)


def alpha32(alpha_host, alpha_dev=None):
    a = np.float32(alpha_host)
    return a if alpha_dev is None else np.float32(a * np.float32(alpha_dev))


def sgemm_accepts(got, acc, alpha, c0=None):
    """element-wise masks (two_step, fused) of got against the two accepted forms of alpha * acc (+ c0); without c0 both are the
    one fp32 multiply.  acc: the fp32 chain (or slab sum), alpha: fp32"""
    got, acc = np.asarray(got, np.float32), np.asarray(acc, np.float32)
    alpha = np.float32(alpha)
    prod = (acc * alpha).astype(np.float32)
    if c0 is None:
        m = got == prod
        return m, m
    c0 = np.asarray(c0, np.float32)
    two = got == (c0 + prod).astype(np.float32)
    # fma: acc * alpha is exact in fp64 (48 bits); the fp64 sum with c0 is rounded once more on its way to fp32, so the fp32
    # neighbours of a sum that sits on an fp32 rounding boundary are both taken
    s = acc.astype(np.float64) * np.float64(alpha) + c0.astype(np.float64)
    fused = np.zeros(got.shape, bool)
    for t in (s, np.nextafter(s, np.inf), np.nextafter(s, -np.inf)):
        fused |= got == t.astype(np.float32)
    return two, fused


def splitk_chain(A, B):
    """uniir_sgemm_splitk's un-scaled sum: per-slice chains added in slice order in fp32"""
    M, K = A.shape
    N = B.shape[1]
    _, kslice, used = splitk_plan(M, N, K)
    part = None
    for s in range(used):
        sl = chain(A[:, s * kslice:min(K, (s + 1) * kslice)], B[s * kslice:min(K, (s + 1) * kslice)])
        part = sl if part is None else (part + sl).astype(np.float32)
    return part


# ---------------------------------------------------------------------------------------------------------- cross-entropy statistics
def _first_argmax(v):
    """first index of the row maximum (torch.max semantics), v [rows][n]"""
    v = torch.as_tensor(v)
    n = v.shape[1]
    idx = torch.arange(n)[None, :].expand_as(v)
    return torch.where(v == v.max(1, keepdim=True).values, idx, torch.full_like(idx, n)).min(1).values


def _lse(z, e_z, depth):
    """z [rows][n] fp64 logits with absolute error e_z -> lse, its bound, softmax p"""
    mx = z.max(1, keepdim=True).values
    ex = (z - mx).exp()
    tot = ex.sum(1, keepdim=True)
    p = ex / tot
    rel_tot = (p * (e_z + EPS32 * (z - mx).abs())).sum(1, keepdim=True) + e_z.max(1, keepdim=True).values + R_EXP + gamma(depth)
    lse = mx + tot.log()
    e_lse = rel_tot + R_LOG * tot.log().abs() + EPS32 * lse.abs()
    return lse[:, 0], e_lse[:, 0], p


def _mean(v, e_v, n_depth):
    n = v.shape[0]
    m = v.mean()
    return m, e_v.mean() + gamma(n_depth) * v.abs().mean() + (R_DIV + 2 * EPS32) * m.abs()


@_margin
def infonce_fwd(score, toff):
    """score [b][B]: the fp32 logits (bit-exact against the chain, checked apart) -> lse, row_loss, hit (exact), loss, acc (exact
    count / b up to the division)"""
    z = torch.as_tensor(score).double()
    b, B = z.shape
    zero = torch.zeros_like(z)
    lse, e_lse, _ = _lse(z, zero, block_depth(B))
    t = toff + torch.arange(b)
    rl = lse - z[torch.arange(b), t]
    e_rl = e_lse + EPS32 * rl.abs()
    hit = (_first_argmax(torch.as_tensor(score)) == t).double()
    loss, e_loss = _mean(rl, e_rl, block_depth(b))
    acc = hit.mean()
    return {"lse": (lse, e_lse), "row_loss": (rl, e_rl), "hit": (hit, torch.zeros_like(hit)), "loss": (loss, e_loss),
            "acc": (acc, R_DIV * acc.abs())}


def _softmax_grad(z, lse, onehot, gmul, rel_gmul):
    """(exp(z - lse) - onehot) * gmul with its bound (z, lse exact inputs)"""
    a = z - lse[:, None]
    p = a.exp()
    G = (p - onehot) * gmul
    e = abs(gmul) * (p * (EPS32 * a.abs() + R_EXP) + EPS32 * (p - onehot).abs()) + (EPS32 + rel_gmul) * G.abs()
    return G, e


@_margin
def infonce_bwd(q, all_p, scale, score, lse, dloss, toff):
    """score, lse: the forward's fp32 outputs (inputs here).  -> G, dq, d_all_p, dscale"""
    q, P, z, lse = (torch.as_tensor(t).double() for t in (q, all_p, score, lse))
    b, B = z.shape
    s = float(scale)
    onehot = torch.zeros(b, B, dtype=torch.float64)
    onehot[torch.arange(b), toff + torch.arange(b)] = 1.0
    G, e_G = _softmax_grad(z, lse, onehot, float(dloss) / b, R_DIV)
    dq = s * (G @ P)
    e_dq = abs(s) * (e_G @ P.abs() + gamma(B + 2) * (G.abs() @ P.abs()))
    dp = s * (G.t() @ q)
    e_dp = abs(s) * (e_G.t() @ q.abs() + gamma(b + 2) * (G.abs().t() @ q.abs()))
    gz = G * z
    dscale = gz.sum() / s
    e_ds = ((e_G * z.abs() + EPS32 * gz.abs()).sum() + gamma(block_depth(B) + block_depth(b)) * gz.abs().sum()) / abs(s) \
        + R_DIV * dscale.abs()
    return {"G": (G, e_G), "dq": (dq, e_dq), "d_all_p": (dp, e_dp), "dscale": (dscale, e_ds)}


# --------------------------------------------------------------------------------------------------------------- hard negatives
def _hn_vectors(p, n, N, I):
    """[b][C][dim]: p_i, the N negatives of row i, then I more copies of p_i (the reference's quirk: its in-batch entries of row i
    are p_i itself)"""
    b, dim = p.shape
    parts = [p[:, None, :]]
    if N:
        parts.append(n.reshape(b, N, dim))
    if I:
        parts.append(p[:, None, :].expand(b, I, dim))
    return torch.cat(parts, 1)


@_margin
def hardneg_fwd(q, p, n, scale, N, I, got_logits=None):
    """-> logits (from q, p, n), and from the kernel's own fp32 logits got_logits (the reference's when None): lse, row_loss, hit"""
    q, p = torch.as_tensor(q).double(), torch.as_tensor(p).double()
    n = torch.as_tensor(n).double() if N else None
    b, dim = q.shape
    V = _hn_vectors(p, n, N, I)
    s = float(scale)
    dots = torch.einsum("bd,bcd->bc", q, V)
    mags = torch.einsum("bd,bcd->bc", q.abs(), V.abs())
    logits = dots * s
    e_log = abs(s) * gamma(wave_depth(dim) + 1) * mags + EPS32 * logits.abs()
    z32 = torch.as_tensor(got_logits) if got_logits is not None else logits.float()
    z = z32.double()
    C = z.shape[1]
    lse, e_lse, _ = _lse(z, torch.zeros_like(z), block_depth(C))
    rl = lse - z[:, 0]
    hit = (_first_argmax(z32) == 0).double()
    return {"logits": (logits, e_log), "lse": (lse, e_lse), "row_loss": (rl, e_lse + EPS32 * rl.abs()),
            "hit": (hit, torch.zeros_like(hit))}


@_margin
def hardneg_bwd(q, p, n, scale, logits, lse, dloss, N, I, dp0=None, dscale0=0.0):
    """logits, lse: the forward's fp32 outputs.  -> dq, dn (written), dp, dscale (added onto dp0 / dscale0)"""
    q, p, z, lse = (torch.as_tensor(t).double() for t in (q, p, logits, lse))
    n = torch.as_tensor(n).double() if N else None
    b, dim = q.shape
    C = 1 + N + I
    s = float(scale)
    V = _hn_vectors(p, n, N, I)
    onehot = torch.zeros(b, C, dtype=torch.float64)
    onehot[:, 0] = 1.0
    g = float(dloss) / b
    D, e_D = _softmax_grad(z, lse, onehot, g, R_DIV)             # d loss / d logit
    dl, e_dl = D * s, abs(s) * e_D + EPS32 * (D * s).abs()       # d loss / d <q, v_c>
    dq = torch.einsum("bc,bcd->bd", dl, V)
    e_dq = torch.einsum("bc,bcd->bd", e_dl, V.abs()) + gamma(C + 1) * torch.einsum("bc,bcd->bd", dl.abs(), V.abs())
    own = torch.ones(C, dtype=torch.bool)
    own[1:1 + N] = False
    dp0 = torch.zeros(b, dim, dtype=torch.float64) if dp0 is None else torch.as_tensor(dp0).double()
    w = dl[:, own].sum(1, keepdim=True)
    wa = dl[:, own].abs().sum(1, keepdim=True)
    dp = dp0 + w * q
    e_dp = (e_dl[:, own].sum(1, keepdim=True) + EPS32 * wa) * q.abs() + gamma(1 + I + 1) * (dp0.abs() + wa * q.abs())
    out = {"dq": (dq, e_dq), "dp": (dp, e_dp)}
    if N:
        dn = dl[:, 1:1 + N, None] * q[:, None, :]
        out["dn"] = (dn, e_dl[:, 1:1 + N, None] * q.abs()[:, None, :] + EPS32 * dn.abs())
    dz = D * z
    tot = dz.sum() / s
    e_tot = ((e_D * z.abs() + EPS32 * dz.abs()).sum() + gamma(C + -(-b // 256) + 9) * dz.abs().sum()) / abs(s) + R_DIV * tot.abs()
    ds0 = float(dscale0)
    out["dscale"] = (torch.tensor(ds0, dtype=torch.float64) + tot, e_tot + EPS32 * (abs(ds0) + tot.abs()))
    return out


# ------------------------------------------------------------------------------------------------------------------------ softce
@_margin
def softce(sim, sim_m, temp, ids_row, ids_all, alpha, gscale, dloss=None):
    """sim, sim_m [b][n]; temp a float or None (1); alpha, gscale floats as passed (fp32); dloss float or None.
    -> row_loss, hit (exact), dsim, row_dtemp"""
    s32 = torch.as_tensor(sim)
    s, sm = s32.double(), torch.as_tensor(sim_m).double()
    b, n = s.shape
    T = 1.0 if temp is None else float(np.float32(temp))
    alpha, gscale = float(np.float32(alpha)), float(np.float32(gscale))
    dep = block_depth(n)
    rz = R_DIV if temp is not None else 0.0
    z, zm = s / T, sm / T
    e_z, e_zm = rz * z.abs(), rz * zm.abs()
    lse, e_lse, p = _lse(z, e_z, dep)
    lse_m, _, pm = _lse(zm, e_zm, dep)
    lsm = z - lse[:, None]
    e_lsm = e_z + e_lse[:, None] + EPS32 * lsm.abs()
    mxm = zm.max(1, keepdim=True).values
    rel_pm = 2 * (e_zm + e_zm.max(1, keepdim=True).values + EPS32 * (zm - mxm).abs()) + 2 * R_EXP + gamma(dep) + R_DIV + 3 * EPS32
    pos = (torch.as_tensor(ids_all)[None, :] == torch.as_tensor(ids_row)[:, None]).double()
    npos = pos.sum(1, keepdim=True)
    inv_pos = torch.where(npos > 0, 1.0 / npos.clamp_min(1.0), torch.zeros_like(npos))
    hard = (1.0 - alpha) * pos * inv_pos
    tgt = alpha * pm + hard
    e_t = abs(alpha) * pm * rel_pm + hard.abs() * (R_DIV + 2 * EPS32) + EPS32 * tgt.abs()
    lt = lsm * tgt
    loss = -lt.sum(1)
    e_loss = (e_lsm * tgt.abs() + lsm.abs() * e_t + e_lsm * e_t + EPS32 * lt.abs()).sum(1) + gamma(dep) * lt.abs().sum(1)
    gs = gscale * (1.0 if dloss is None else float(np.float32(dloss)))
    g = (lsm.exp() - tgt) * gs
    e_g = abs(gs) * (lsm.exp() * (e_lsm + R_EXP) + e_t + EPS32 * (lsm.exp() - tgt).abs()) + 2 * EPS32 * g.abs()
    dsim = g / T
    e_dsim = e_g / abs(T) + rz * dsim.abs()
    gz = g * z
    dtemp = -gz.sum(1) / T
    e_dtemp = ((e_g * z.abs() + g.abs() * e_z + EPS32 * gz.abs()).sum(1) + gamma(dep) * gz.abs().sum(1)) / abs(T) + rz * dtemp.abs()
    v32 = s32 if temp is None else torch.from_numpy((s32.numpy() / np.float32(temp)).astype(np.float32))
    am = _first_argmax(v32)
    hit = pos[torch.arange(b), am]
    return {"row_loss": (loss, e_loss), "hit": (hit, torch.zeros_like(hit)), "dsim": (dsim, e_dsim),
            "row_dtemp": (dtemp, e_dtemp)}


# ------------------------------------------------------------------------------------------------------------- select, fuse, pool
@_margin
def select_normalize(emb, idx):
    """-> out [rows][dim], inv_norm [rows]"""
    x = torch.as_tensor(emb).double()
    if idx is not None:
        x = x[torch.as_tensor(idx).long()]
    dim = x.shape[1]
    nrm = (x * x).sum(1, keepdim=True).sqrt().clamp_min(1e-12)
    rel = 0.5 * gamma(wave_depth(dim) + 1) + R_SQRT + R_DIV + EPS32
    out, inv = x / nrm, (1.0 / nrm)[:, 0]
    return {"out": (out, rel * out.abs()), "inv_norm": (inv, rel * inv.abs())}


@_margin
def select_normalize_bwd(out, inv_norm, dout, idx, demb0):
    """demb0 [n][dim] prior contents -> demb = demb0 with (dout_i - out_i <out_i, dout_i>) inv_norm_i added to row idx[i], every i"""
    y, iv, dy, d0 = (torch.as_tensor(t).double() for t in (out, inv_norm, dout, demb0))
    rows, dim = y.shape
    idx = torch.arange(rows) if idx is None else torch.as_tensor(idx).long()
    s = (y * dy).sum(1, keepdim=True)
    e_s = gamma(wave_depth(dim) + 1) * (y * dy).abs().sum(1, keepdim=True)
    t = (dy - y * s) * iv[:, None]
    mag = (dy.abs() + (y * s).abs()) * iv.abs()[:, None]
    e_t = y.abs() * e_s * iv.abs()[:, None] + 3 * EPS32 * mag
    cnt = torch.zeros(d0.shape[0], dtype=torch.float64).index_add_(0, idx, torch.ones(rows, dtype=torch.float64))
    demb = d0.clone().index_add_(0, idx, t)
    summ = d0.abs().index_add_(0, idx, t.abs())
    bound = torch.zeros_like(d0).index_add_(0, idx, e_t) + (cnt[:, None] + 1) * EPS32 / (1 - (cnt[:, None] + 1) * EPS32) * summ
    return {"demb": (demb, bound)}


@_margin
def fuse_embeddings(txt, img, tmask, imask):
    t, im = torch.as_tensor(txt).double(), torch.as_tensor(img).double()
    e = t * torch.as_tensor(tmask).double()[:, None] + im * torch.as_tensor(imask).double()[:, None]
    return {"emb": (e, EPS32 * e.abs())}


@_margin
def fuse_embeddings_bwd(demb, tmask, imask):
    """exact: a product with 0 or 1"""
    d = torch.as_tensor(demb).double()
    dt, di = d * torch.as_tensor(tmask).double()[:, None], d * torch.as_tensor(imask).double()[:, None]
    return {"dtxt": (dt, torch.zeros_like(dt)), "dimg": (di, torch.zeros_like(di))}


@_margin
def meanpool_fwd(x):
    """x [n][T][W] -> out [n][W]"""
    x = torch.as_tensor(x).double()
    T = x.shape[1]
    return {"out": (x.mean(1), (gamma(T + 1) + R_DIV) * x.abs().mean(1))}


@_margin
def meanpool_bwd(dout, T):
    d = torch.as_tensor(dout).double()
    dx = (d / T)[:, None, :].expand(d.shape[0], T, d.shape[1])
    return {"dx": (dx, (R_DIV + EPS32) * dx.abs())}


# --------------------------------------------------------------------------------------------------------------------- optimizer
@_margin
def adamw_step(p, g, m, v, lr, b1, b2, eps, wd, step, grad_scale=1.0):
    """one step of torch.optim.AdamW's single-tensor form from the given state (all scalars as passed: fp32) -> param, exp_avg,
    exp_avg_sq.  The bf16 shadow is bf16(param as stored), bit for bit, and is checked against the kernel's own param."""
    p, g, m, v = (torch.as_tensor(t).double() for t in (p, g, m, v))
    lr, b1, b2, eps, wd, gs = (float(np.float32(t)) for t in (lr, b1, b2, eps, wd, grad_scale))
    g1 = g * gs
    m1 = m * b1 + g1 * (1.0 - b1)
    e_m = 4 * EPS32 * ((m * b1).abs() + (g1 * (1.0 - b1)).abs())
    v1 = v * b2 + g1 * g1 * (1.0 - b2)
    e_v = 6 * EPS32 * v1.abs()
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    rel_bc1 = R_POW * (b1 ** step) / bc1 + EPS32
    rel_bc2s = 0.5 * (R_POW * (b2 ** step) / bc2 + EPS32) + R_POW
    p1 = p * (1.0 - lr * wd)
    e_p1 = 3 * EPS32 * p1.abs()
    root = v1.sqrt() / math.sqrt(bc2)
    denom = root + eps
    # sqrt halves v's relative error; where v1 is tiny against its own bound the absolute form sqrt(e_v) covers it
    e_root = torch.minimum(root * (0.5 * e_v / v1.clamp_min(1e-300)), (e_v / bc2).sqrt()) + root * (R_SQRT + R_DIV + rel_bc2s)
    e_den = e_root + EPS32 * denom
    upd = (lr / bc1) * (m1 / denom)
    e_upd = (lr / bc1) * (e_m / denom + m1.abs() * e_den / (denom * (denom - e_den).clamp_min(1e-300))) \
        + upd.abs() * (2 * R_DIV + 2 * EPS32 + rel_bc1)
    pn = p1 - upd
    return {"param": (pn, e_p1 + e_upd + EPS32 * pn.abs()), "exp_avg": (m1, e_m), "exp_avg_sq": (v1, e_v)}


@_margin
def ema_update(pm, p, momentum):
    pm, p = torch.as_tensor(pm).double(), torch.as_tensor(p).double()
    mo = float(np.float32(momentum))
    r = pm * mo + p * (1.0 - mo)
    return {"param_m": (r, 4 * EPS32 * ((pm * mo).abs() + (p * (1.0 - mo)).abs()))}
