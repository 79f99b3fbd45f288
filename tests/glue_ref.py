"""References of the tower glue kernels (csrc/elementwise.hip, uniir_vit_assemble_f32, uniir_pool_inv_norms) and their bounds.

Not a test module and free of any GPU call: tests/test_glue_paths_gpu.py compares every kernel path against it, tests/test_glue_ref.py
checks on the CPU that the references agree with independent torch formulations, that an fp32 restatement of every bounded case stays
at half of its bound, and that planted defects do not pass.  Every function restates one operation as include/uniir_hip.h and the
kernels' comments state it.  The exact references are written with torch operations that are exact on any device (indexing, one fp32
addition, the IEEE conversions), so the large grid-stride cases can be evaluated where their tensors live.

Exact operations (compared bit for bit): patchify (k = c P P + py P + px, zeros in [3 P P, kpad), round-to-nearest-even bf16),
vit_assemble / vit_assemble_f32 / text_embed / text_embed_packed (one fp32 addition), eot (first arg-max), last_row, gather_rows,
scatter_rows and unpad_add (+= onto the prior contents), cast_pad_rows{,_f16}, cast_bf16_to_f32, the dropout masks, dropout_bf16
(fl32(x * fl32(m * rowscale)) rounded to bf16), vit_assemble_bwd's dpatch, and the position / class gradients: one thread adds its
items in ascending order starting from 0, then adds that sum onto the prior contents -- chain_sum.  pool_inv_norms is the pinned chain
of oracle/oracle.c.

Dropout masks (common.h: "element idx of a call with seed s is kept iff fmix32(idx * golden ^ s) >= p * 2^32"): golden = 0x9E3779B1,
fmix32 is MurmurHash3's finaliser, all in uint32; the threshold is the fp32 product p * 2^32 cut to an integer and capped at
4294967040 (the largest fp32 below 2^32); kept elements carry ks = fl32(1 / fl32(1 - p)).  The element index is row * cols + col of
the LOGICAL tensor: through row_map for the packed forms, without the pitch for the bf16 form.  dropout_f32 is
resid + x * fl32(m * rowscale): the build contracts floating-point expressions, so the addition may be fused with the product;
both forms are accepted element by element (dropout_forms), as fp32_ref.sgemm_accepts does for alpha * acc + c.

Sums (colsum_bf16, the token-embedding gradient).  On integer data whose absolute sum stays below 2^24 every order is exact: bound 0.
Otherwise gamma(depth) * sum |terms| with the depth of the kernels' summation trees:
  colsum    a lane adds ceil(rpb / 4) rows, the four lanes add as a tree (2); one row block adds onto the destination (1); several
            store partials that partial_reduce adds as 32 chunks of ceil(gy / 32) parts, the chunk sums in a chain of 32, then the
            destination (1) -- or, without scratch, gy atomic additions in any order: colsum_depth.
  dtok      tokd_sum: four quarters of ceil(cnt / 4) rows (the first addition onto 0 is exact), the quarter sums in a chain of 3:
            ceil(cnt / 4) + 2, then the destination (1); a long id adds its slices' partials in a chain (nslices) first; the atomic
            kernels add cnt rows in any order onto the destination: cnt + 1.  tokd_depth.

Conversions.  Expected: torch's CPU cast (IEEE round-to-nearest-even with gradual underflow).  cast_inputs builds, from all 65536
target bit patterns v, v itself, the midpoint between v and its successor (a tie) and the midpoint -/+ one fp32 ulp; the successor of
the largest finite value is the power of two above it, so the last tie rounds to infinity.  A NaN must stay a NaN (any payload).  An
input in fp32's subnormal range (|x| < 2^-126) may give a same-signed zero instead (hardware converts may flush their input).

Device-function budgets (relative, per call, fp32_ref's rule: the documented HIP accuracy with a 4x margin -- no accuracy table ships
with ROCm): v_exp_f32 through __expf 1 ulp -> EXP_ULP = 4 (fp32_ref.R_EXP); v_rcp_f32 1 ulp -> RCP_ULP = 4; tanhf 2 ulp (the HIP
programming guide's table, the same figure CUDA documents) -> TANH_ULP = 8.  MARGIN = 2 on top, like every bound of fp32_ref.
  __expf(a) is exp2(fl(a * fl(log2 e))): the two roundings move the base-2 argument by up to 2 |a| log2(e) EPS32, i.e. the result by
  the relative 2 ln 2 |a| log2(e) EPS32 = 2 |a| EPS32 -- the budget grows with the argument.  The argument itself carries its own
  roundings (QuickGELU: the fp32 constant 1.702f and the product, 2 EPS32 |a|; erf-GELU: -0.5 x * x, one rounding).
  QuickGELU  y = x * rcp(1 + E), E = exp(-t), t = 1.702 x:  rel(E) = R_EXP + 4 |t| EPS32;  rel(s) = rel(E) E / (1 + E) + EPS32 +
             R_RCP;  |y^ - y| <= |y| (rel(s) + EPS32) + |x| TINY32  (s, or E, in fp32's subnormal range may be flushed).
  erf-GELU   y = x * Phi(x), Phi from Abramowitz-Stegun 7.1.26: |erf error| < 1.5e-7 (common.h), 0.75e-7 on Phi -- an ABSOLUTE error of
             Phi, so |x| * 0.75e-7 on y: the tail's relative error is large by design.  The fp32 evaluation adds: t = rcp(fma):
             rel R_RCP + 2 EPS32; the Horner polynomial (coefficients below 1.5 in magnitude, |p'| <= 12 on (0, 1]): 8 EPS32 +
             12 t rel(t) absolute; E = exp(-x^2 / 2): rel R_EXP + 3 (x^2 / 2) EPS32; q = 0.5 t p E: q (rel(t) + rel(E) + 3 EPS32) +
             0.5 t E e_p; Phi = 1 - q or q: one more rounding; y = x Phi: one more, and |x| TINY32 for a flushed E or q.
  ReLU       exact.  NaN gives NaN in all three; infinities follow the fp64 formula (x * sigma(-inf) = -inf * 0 = NaN).
  act_fwd rounds to bf16: MARGIN * bf16_bound(ref, e) + TINY32, like fp32_ref's 16-bit outputs.
  tanh_fwd   R_TANH |tanh x|;  tanh_bwd dx = dy (1 - y^2): EPS32 (y^2 + |1 - y^2|) |dy| + EPS32 |dx| (contracted or not).
"""
import numpy as np
import torch

from fp32_ref import (EPS32, MARGIN, R_EXP, TINY32, _exact_int_sum, _first_argmax, bf16_bound, check, gamma,  # noqa: F401
                      violations, worst_ratio)

BF16, F16 = torch.bfloat16, torch.float16
RCP_ULP, TANH_ULP = 4, 8
R_RCP, R_TANH = 2.0 * EPS32 * RCP_ULP, 2.0 * EPS32 * TANH_ULP
AS_CDF_ERR = 0.75e-7          # half of 7.1.26's 1.5e-7 on erf
QUICK_GELU, ERF_GELU, RELU = 0, 1, 2
TOKD_SORT = 4096


def _with_margin(b):
    return torch.where(b > 0, MARGIN * b + TINY32, torch.zeros_like(b))


def ibits(t):
    """the integer view of a tensor's bit patterns"""
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.dtype.itemsize])


def assert_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w = ibits(got), ibits(want.to(got.device))
    if not torch.equal(g, w):
        bad = torch.nonzero(g != w)
        first = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {g.numel()} elements differ in their bits; first at {first}: got "
                             f"{float(got[first])} ({int(g[first]) & 0xffffffff:#x}), expected {float(want[first])} "
                             f"({int(w[first]) & 0xffffffff:#x})")


# ------------------------------------------------------------------------------------------------------------------ exact: forward
def patchify(img, P, kpad):
    """img fp32 [n][3][res][res] -> bf16 [n g g][kpad], k = c P P + py P + px, zeros from 3 P P on"""
    n, ch, res, _ = img.shape
    g = res // P
    rows = img.reshape(n, ch, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(n * g * g, ch * P * P)
    out = torch.zeros(n * g * g, kpad, dtype=img.dtype, device=img.device)
    out[:, :ch * P * P] = rows
    return out if img.dtype == torch.float64 else out.to(BF16)          # (float64 in: the unrounded operation, tests/tower_ref.py)


def vit_assemble(po, cls, pos, n, T):
    """po bf16 or fp32 [n (T - 1)][w], cls [w], pos [T][w] -> x fp32 [n T][w] = (t == 0 ? cls : po[n][t - 1]) + pos[t]"""
    w = cls.numel()
    row = torch.arange(n * T, device=po.device)
    t, im = row % T, row // T
    src = (po if po.dtype == torch.float64 else po.float())[(im * (T - 1) + (t - 1)).clamp_min(0)]
    src = torch.where((t == 0)[:, None], cls[None, :].expand(n * T, w), src)
    return src + pos[t]


def vit_assemble_bwd(dx, n, T, dclass0, dpos0):
    """dx fp32 [n T][w] -> dpatch bf16 [n (T - 1)][w], dclass [w], dpos [T][w] (chains over the items onto the prior contents)"""
    w = dx.shape[1]
    d = dx.view(n, T, w)
    s = chain_sum(d)
    dpatch = d[:, 1:].reshape(n * (T - 1), w)
    return {"dpatch": dpatch if dx.dtype == torch.float64 else dpatch.to(BF16), "dclass": dclass0 + s[0], "dpos": dpos0 + s}


def chain_sum(terms, live=None):
    """fp32 sum over dim 0 as one thread takes it: s = 0, s = s + terms[i] in ascending i (only where live[i], when given)"""
    s = torch.zeros_like(terms[0])
    for i in range(terms.shape[0]):
        s = s + terms[i] if live is None else torch.where(live[i], s + terms[i], s)
    return s


def clamp_ids(text, vocab):
    return text.long().clamp(0, vocab - 1)


def text_embed(text, tok, pos, vocab):
    """text int32 [n][ctx] -> x fp32 [n ctx][w] = tok[clamped id] + pos[t], eot [n] = first arg-max of the row"""
    n, ctx = text.shape
    x = tok[clamp_ids(text, vocab)] + pos[None, :ctx]
    return x.reshape(n * ctx, -1), _first_argmax(text.cpu()).to(torch.int32)


def row_offsets(lens):
    off = torch.zeros(lens.numel() + 1, dtype=torch.int32, device=lens.device)
    off[1:] = torch.cumsum(lens, 0)
    return off


def live_mask(lens, ctx):
    return torch.arange(ctx, device=lens.device)[None, :] < lens[:, None]


def text_embed_packed(text, tok, pos, vocab, lens):
    """-> x fp32 [sum lens][w]: item m's tokens 0 .. lens[m] - 1 at rows row_off[m] ..; last_row [n] = row_off[m + 1] - 1"""
    n, ctx = text.shape
    x, _ = text_embed(text, tok, pos, vocab)
    off = row_offsets(lens)
    return x.view(n, ctx, -1)[live_mask(lens, ctx)], (off[1:] - 1).to(torch.int32)


def text_dpos(dx, n, ctx, dpos0, lens=None):
    """dpos[t] = dpos0[t] + chain over the items of dx[item][t]; packed (lens given): dx [sum lens][w], items shorter than t + 1 skipped"""
    w = dx.shape[1]
    if lens is None:
        return dpos0 + chain_sum(dx.view(n, ctx, w))
    m = live_mask(lens, ctx)
    dense = torch.zeros(n, ctx, w, dtype=dx.dtype, device=dx.device)
    dense[m] = dx
    return dpos0 + chain_sum(dense, m[:, :, None])


def row_index(n, seq, idx, device="cpu"):
    r = torch.arange(n, device=device) * seq
    return r if idx is None else r + idx.long()


def gather_rows(x, idx, n, seq):
    return x[row_index(n, seq, idx, x.device)]


def scatter_rows(dout, idx, dx0, seq):
    """dx0 with dout[i] added to row i seq + idx[i] (rows are distinct); every other row keeps its bits"""
    r = row_index(dout.shape[0], seq, idx, dout.device)
    dx = dx0.clone()
    dx[r] = dx0[r] + dout
    return dx


def cast_pad_rows(src, ld, dtype):
    rows, cols = src.shape
    out = torch.zeros(rows, ld, dtype=torch.float32, device=src.device)
    out[:, :cols] = src
    return out.to(dtype)


def bf16_to_f32(x):
    return (x.view(torch.int16).to(torch.int32) << 16).view(torch.float32)


# ----------------------------------------------------------------------------------------------------------------------- dropout
def drop_hash(idx, seed):
    with np.errstate(over="ignore"):
        h = (np.asarray(idx).astype(np.uint32) * np.uint32(0x9E3779B1)) ^ np.uint32(seed)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    return h


def drop_threshold(p):
    return int(min(np.float32(p) * np.float32(4294967296.0), np.float32(4294967040.0)))


def keep_scale(p):
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def drop_mask(rows, cols, p, seed, row_map=None, always_hash=False):
    """fp32 numpy [rows][cols]: ks where element row_map[row] * cols + col of the logical tensor is kept, 0 elsewhere.  p == 0 keeps
    everything at 1 (uniir_dropout_mask hashes all the same: threshold 0, ks 1 -- the same mask)"""
    if p == 0 and not always_hash:
        return np.ones((rows, cols), np.float32)
    r = np.arange(rows, dtype=np.int64) if row_map is None else np.asarray(row_map, np.int64)
    idx = (r[:, None] * cols + np.arange(cols, dtype=np.int64)[None, :]) & 0xFFFFFFFF
    keep = drop_hash(idx, seed) >= np.uint32(drop_threshold(p))
    return np.where(keep, keep_scale(p), np.float32(0.0)).astype(np.float32)


def drop_factor(mask, rowscale=None, div=1):
    """fl32(mask * rowscale[row / div])"""
    if rowscale is None:
        return mask
    rs = np.asarray(rowscale, np.float32)[np.arange(mask.shape[0]) // div]
    return (mask * rs[:, None]).astype(np.float32)


def dropout_forms(x, factor, resid=None):
    """the accepted fp32 values of resid + x * factor: [two roundings, fused (with its fp32 neighbours where the fp64 sum sits on a
    rounding boundary)]; without resid the one product"""
    x, factor = np.asarray(x, np.float32), np.asarray(factor, np.float32)
    prod = (x * factor).astype(np.float32)
    if resid is None:
        return [prod]
    resid = np.asarray(resid, np.float32)
    s = x.astype(np.float64) * factor.astype(np.float64) + resid.astype(np.float64)
    return [(resid + prod).astype(np.float32)] + [t.astype(np.float32) for t in (s, np.nextafter(s, np.inf), np.nextafter(s, -np.inf))]


def to_bf16_np(a):
    """numpy fp32 -> the bf16 bit patterns (uint16) of torch's CPU cast"""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(BF16).view(torch.int16).numpy().view(np.uint16)


def dropout_accepts(got, forms, bf16=False):
    """-> (ok mask, elements equal to the two-rounding form only, to a fused form only, to both); got: numpy fp32, or the uint16 bits
    of bf16"""
    conv = to_bf16_np if bf16 else (lambda a: a.view(np.uint32))
    g = np.asarray(got) if bf16 else np.asarray(got, np.float32).view(np.uint32)
    two = g == conv(forms[0])
    fused = np.zeros(g.shape, bool)
    for f in forms[1:]:
        fused |= g == conv(f)
    return two | fused, int((two & ~fused).sum()), int((fused & ~two).sum()), int((two & fused).sum())


def dropout_bf16(x, factor):
    """x bf16 torch [rows][cols], factor numpy fp32 -> bf16 of fl32(x * factor)"""
    return (x.float() * torch.from_numpy(factor).to(x.device)).to(BF16)


# ------------------------------------------------------------------------------------------------------------------------- sums
def colsum_depth(rpb, gy):
    lane = -(-rpb // 4) + 2
    if gy == 1:
        return lane + 1
    return lane + max(gy, -(-gy // 32) + 32) + 1


def tokd_depth(cnt, fixed, nslices=0):
    """per id (cnt: int64 tensor of bucket sizes; nslices: the row ranges of TOKD_SORT rows a long id's partials are added over)"""
    if not fixed:
        return cnt + 1
    short = -(-cnt.clamp_max(TOKD_SORT) // 4) + 2
    return short + torch.where(cnt > TOKD_SORT, torch.full_like(cnt, nslices), torch.zeros_like(cnt)) + 1


def _sum_bound(terms_abs, prior, depth, exact):
    b = gamma(depth) * (terms_abs + prior.abs())
    return torch.where(exact, torch.zeros_like(b), _with_margin(b))


def colsum(x, out0, depth):
    """x bf16 [rows][cols] (the logical view), out0 [cols] -> (out0 + column sums in fp64, bound)"""
    t, p = x.double().cpu(), out0.double().cpu()
    return p + t.sum(0), _sum_bound(t.abs().sum(0), p, float(depth), _exact_int_sum(t, p))


def token_counts(text, vocab, lens=None):
    ids = clamp_ids(text, vocab)
    if lens is not None:
        ids = ids[live_mask(lens, text.shape[1])]
    return torch.bincount(ids.flatten(), minlength=vocab)


def dtok(text, dx, vocab, dtok0, fixed, lens=None, nslices=0):
    """dtok0 [vocab][w] with every dx row added to the row of its (clamped) id -> (fp64 reference, bound).  dx [n ctx][w], or packed
    [sum lens][w] with lens"""
    ids = clamp_ids(text.cpu(), vocab)
    ids = ids[live_mask(lens.cpu(), text.shape[1])] if lens is not None else ids.flatten()
    d, p = dx.double().cpu(), dtok0.double().cpu()
    ref = p.clone().index_add_(0, ids, d)
    mag = torch.zeros_like(p).index_add_(0, ids, d.abs())
    cnt = torch.bincount(ids, minlength=vocab)
    ints = (d == d.round()).all() & (p == p.round()).all()
    exact = (mag + p.abs() < 2.0 ** 24) & ints
    depth = tokd_depth(cnt, fixed, nslices).double()[:, None]
    b = depth * EPS32 / (1.0 - depth * EPS32) * (mag + p.abs())
    return ref, torch.where(exact, torch.zeros_like(b), _with_margin(b))


def inv_norms(x_f16):
    """the pinned chain of oracle.c: sequential fp32 sum of squares, 1.0 / sqrtf in double, 0 for an all-zero row"""
    from oracle import c_oracle
    return torch.from_numpy(c_oracle.inv_norms(x_f16.cpu().view(torch.int16).numpy().view(np.uint16)))


# --------------------------------------------------------------------------------------------------------------------- conversions
def _f32(bits):
    return torch.from_numpy(np.asarray(bits, np.uint32).view(np.float32).copy())


def cast_inputs(dtype):
    """fp32 inputs built from all 65536 bit patterns of dtype: the value, the tie above it, the tie -/+ one fp32 ulp; plus a few
    fp32 subnormals of both signs"""
    v = np.arange(65536, dtype=np.uint32)
    sub = np.array([0x00000001, 0x00400000, 0x007FFFFF, 0x80000001, 0x80400000, 0x807FFFFF], np.uint32)
    if dtype == BF16:
        base = v << 16
        parts = [base, base + 0x7FFF, base + 0x8000, base + 0x8001, sub]
        return _f32(np.concatenate(parts))
    h = torch.from_numpy(v.astype(np.uint16).view(np.int16).copy()).view(F16).float().numpy()
    a = np.abs(h)
    fin = np.isfinite(h)
    a = a[fin]
    sgn = np.where(np.signbit(h[fin]), np.float32(-1), np.float32(1))
    nxt = torch.from_numpy(((v[fin] & 0x7FFF) + 1).astype(np.uint16).view(np.int16).copy()).view(F16).float().numpy()
    nxt = np.where(np.isinf(nxt), np.float32(65536.0), nxt)
    mid = ((a.astype(np.float64) + nxt.astype(np.float64)) / 2).astype(np.float32)          # exact: 12 significant bits
    assert np.array_equal(mid.astype(np.float64) * 2, a.astype(np.float64) + nxt.astype(np.float64))
    parts = [h, sgn * mid, sgn * np.nextafter(mid, np.float32(0)), sgn * np.nextafter(mid, np.float32(np.inf)), sub.view(np.float32)]
    return torch.from_numpy(np.concatenate(parts).astype(np.float32))


def cast_verdict(x, got, dtype):
    """x fp32 inputs, got their conversions (dtype) -> (bad mask, number of fp32-subnormal inputs, how many of them came out as the
    IEEE result, how many as a same-signed zero only)"""
    x, got = x.cpu(), got.cpu()
    want = x.to(dtype)
    g, w = ibits(got), ibits(want)
    ieee = g == w
    nan_ok = torch.isnan(want) & torch.isnan(got)
    sub = (x != 0) & (x.abs() < TINY32)
    zero = sub & (g == torch.where(torch.signbit(x), torch.tensor(-0x8000, dtype=torch.int16), torch.tensor(0, dtype=torch.int16)))
    bad = ~(ieee | nan_ok | zero)
    return bad, int(sub.sum()), int((sub & ieee).sum()), int((zero & ~ieee).sum())


# ---------------------------------------------------------------------------------------------------------------- bounded functions
def act_fwd(x, act):
    """x: fp32 tensor of finite bf16 values -> (fp64 reference of act(x), bound of the bf16 result)"""
    x = x.double()
    ax = x.abs()
    if act == RELU:
        y = x.clamp_min(0.0)
        return y, torch.zeros_like(y)
    if act == QUICK_GELU:
        t = 1.702 * x
        s = torch.sigmoid(t)
        y = x * s
        e_over = torch.exp(-t.clamp_min(-700.0))                       # E; E / (1 + E) = 1 - s
        rel_e = R_EXP + 4.0 * t.abs() * EPS32
        rel_s = rel_e * torch.where(torch.isfinite(e_over), 1.0 - s, torch.ones_like(s)) + EPS32 + R_RCP
        e = y.abs() * (rel_s + EPS32) + ax * TINY32
    else:
        cdf = 0.5 * torch.erfc(-x / 2.0 ** 0.5)
        y = x * cdf
        t = 1.0 / (1.0 + 0.23164189 * ax)
        E = torch.exp(-0.5 * x * x)
        q = 0.5 * torch.erfc(ax / 2.0 ** 0.5)
        rel_t = R_RCP + 2 * EPS32
        rel_e = R_EXP + 3.0 * (0.5 * x * x) * EPS32
        e_p = 8 * EPS32 + 12.0 * t * rel_t
        e_q = q * (rel_t + rel_e + 3 * EPS32) + 0.5 * t * E * e_p
        e_cdf = e_q + EPS32 * cdf + AS_CDF_ERR
        e = ax * e_cdf + EPS32 * y.abs() + ax * TINY32
    e = torch.where(torch.isfinite(e), e, torch.full_like(e, 1e300))          # |x| near fp32's maximum: x^2 overflows nothing in fp64
    return y, _with_margin(bf16_bound(y, e))


def act_special(x, act):
    """the fp64 formula on NaN / +-Inf inputs -> fp64 values (NaN, +-Inf or 0)"""
    x = x.double()
    if act == RELU:
        return torch.where(torch.isnan(x), x, x.clamp_min(0.0))
    if act == QUICK_GELU:
        return x * torch.sigmoid(1.702 * x)
    return x * (0.5 * torch.erfc(-x / 2.0 ** 0.5))


def tanh_fwd(x):
    y = torch.tanh(x.double())
    return y, _with_margin(R_TANH * y.abs())


def tanh_bwd(y, dy):
    y, dy = y.double(), dy.double()
    dx = dy * (1.0 - y * y)
    return dx, _with_margin(EPS32 * (y * y + (1.0 - y * y).abs()) * dy.abs() + EPS32 * dx.abs())
