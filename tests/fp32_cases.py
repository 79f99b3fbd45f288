"""The case tables of tests/test_norm_paths_gpu.py and tests/test_loss_paths_gpu.py, with the builders of their inputs.

Not a test module and free of any GPU call: tests/test_fp32_ref.py walks the same tables on the CPU (an fp32 restatement of every
case at its real shape must stay inside the bound of tests/fp32_ref.py, and the host arithmetic must send every case to the path it
names), the GPU files run them on the kernels.  Builders take the device, so both sides see the same shapes and the same kind of data.
"""
from dataclasses import dataclass

import torch

import fp32_ref as R

NAN32 = 0x7FC00011
NAN16 = 0x7FC1
GUARD = 8             # guard rows behind every tensor


class Buf:
    """a [rows][cols] view of pitch ld at element offset off inside a flat buffer with GUARD rows behind it; every element outside
    the view holds a NaN pattern"""

    def __init__(self, rows, cols, ld=None, dtype=torch.float32, off=0, device="cpu"):
        ld = cols if ld is None else ld
        assert ld >= cols
        self.rows, self.cols, self.ld, self.off, self.dtype = rows, cols, ld, off, dtype
        self.ibits = {2: torch.int16, 4: torch.int32, 8: torch.int64}[dtype.itemsize]
        self.flat = torch.empty(off + (rows + GUARD) * ld, dtype=dtype, device=device)
        self.flat.view(self.ibits).fill_(NAN16 if dtype.itemsize == 2 else NAN32)
        self.view = self.flat[off:].as_strided((rows, cols), (ld, 1))

    def set(self, t):
        self.view.copy_(t.to(self.dtype))
        return self

    def bits(self):
        return self.flat.view(self.ibits)

    def outside_mask(self):
        m = torch.ones(self.flat.numel(), dtype=torch.bool, device=self.flat.device)
        m[self.off:].as_strided((self.rows, self.cols), (self.ld, 1)).fill_(False)
        return m

    def assert_outside_untouched(self, before, what):
        m = self.outside_mask()
        assert torch.equal(self.bits()[m], before[m]), f"{what}: changed outside its extent"

    def assert_all_untouched(self, before, what):
        assert torch.equal(self.bits(), before), f"{what}: written although the call was refused"


# ==================================================================================================================== the norms
@dataclass
class NormCase:
    name: str
    rows: int
    width: int
    rms: bool = False
    xpad: bool = False            # x_stride = 3 * width + 8 instead of width
    outs: str = "both"            # forward: bf16 | f32 | both
    data: str = "randn"           # randn | bigmean | const | zero | gamma0 | intdy (integer dy and dbeta contents)
    bwd: bool = False
    dy_f32: bool = True
    opts: bool = False            # backward: dres with dx_stride = width + 12, dx_bf16, dx_colsum and (LayerNorm) branch_scale -- all on, or all off
    scratch: object = "on"        # on | off | short (one byte less than the launch asks for)
    mix: str = None               # backward: the options one by one instead of `opts` -- letters of r (dres), s (dx_stride = width + 12),
                                  # b (dx_bf16), c (dx_colsum), k (branch_scale); the kernel branches on each of them separately

    def has(self, o):
        return o in self.mix if self.mix is not None else self.opts

    @property
    def path(self):
        nc, exact = R.ln_path(self.width)
        return f"NC{nc}{'e' if exact else 'p'}"

    @property
    def eps(self):
        return 1e-6 if self.rms else 1e-5

    @property
    def x_stride(self):
        return 3 * self.width + 8 if self.xpad else self.width

    @property
    def dx_stride(self):
        return self.width + 12 if self.has("s") else self.width

    @property
    def workgroups(self):
        """of the backward launch, as long as the grid is not clipped to the resident wave (rows <= 1024)"""
        return -(-self.rows // 4)


FWD_WIDTHS = {4: "NC2p", 64: "NC2p", 260: "NC2p", 508: "NC2p", 512: "NC2e", 516: "NC3p", 764: "NC3p", 768: "NC3e", 772: "NC4p",
              1020: "NC4p", 1024: "NC4e", 1028: "NC8p", 1280: "NC8p", 2044: "NC8p", 2048: "NC8e"}
GRID_WIDTHS = {260: "NC2p", 512: "NC2e", 764: "NC3p", 768: "NC3e", 1020: "NC4p", 1024: "NC4e", 2044: "NC8p", 2048: "NC8e"}
ROWS = (1, 3, 4, 5, 37)
OUTS = ("bf16", "f32", "both")
LONG_ROWS = 8231          # > 8 workgroups / CU x 256 CUs x 4 rows: the persistent row loop strides at any occupancy

NORM_FWD = []
for _i, _w in enumerate(FWD_WIDTHS):
    NORM_FWD.append(NormCase(f"ln-fwd-w{_w}", ROWS[_i % 5], _w, xpad=_i % 2 == 1, outs=OUTS[_i % 3]))
for _w in (260, 768):                         # every row count and every output combination once more on one predicated / exact width
    for _i, _r in enumerate(ROWS):
        NORM_FWD.append(NormCase(f"ln-fwd-w{_w}-r{_r}", _r, _w, xpad=_i % 2 == 0, outs=OUTS[(_i + 1) % 3]))
NORM_FWD.append(NormCase("ln-fwd-long-exact", LONG_ROWS, 768))
NORM_FWD.append(NormCase("ln-fwd-long-pred", LONG_ROWS, 764, outs="f32"))
for _i, _w in enumerate(GRID_WIDTHS):
    NORM_FWD.append(NormCase(f"rms-fwd-w{_w}", ROWS[(_i + 2) % 5], _w, rms=True, xpad=_i % 2 == 0, outs=OUTS[_i % 3]))
NORM_FWD.append(NormCase("rms-fwd-long-pred", LONG_ROWS, 260, rms=True, outs="bf16"))
for _d in ("bigmean", "const", "gamma0"):
    NORM_FWD.append(NormCase(f"ln-fwd-{_d}", 5, 764, data=_d))
    NORM_FWD.append(NormCase(f"ln-fwd-{_d}-exact", 5, 768, data=_d))
NORM_FWD.append(NormCase("rms-fwd-zero", 5, 260, rms=True, data="zero"))
NORM_FWD.append(NormCase("rms-fwd-gamma0", 5, 768, rms=True, data="gamma0"))

# The backward has sixteen kernel instances (NC x EXACT x DY_F32).  The options (dres + dx_stride > width, dx_bf16, dx_colsum,
# branch_scale) are run-time arguments of one instance, so two cases per instance -- all options on, all off -- pair every instance
# with both values of every option; 37 rows make 10 workgroups (stored partials).  RMS mode runs the same instances with rms = 1:
# one case per instance, the options alternating.
NORM_BWD = []
for _w in GRID_WIDTHS:
    for _f in (False, True):
        for _o in (False, True):
            NORM_BWD.append(NormCase(f"ln-bwd-w{_w}-{'f32' if _f else 'bf16'}-{'opts' if _o else 'plain'}", 37, _w, bwd=True,
                                     dy_f32=_f, opts=_o, xpad=_o))
for _i, _w in enumerate(GRID_WIDTHS):
    for _f in (False, True):
        NORM_BWD.append(NormCase(f"rms-bwd-w{_w}-{'f32' if _f else 'bf16'}", 37, _w, rms=True, bwd=True, dy_f32=_f,
                                 opts=(_i + _f) % 2 == 0))
# reduction forms: one workgroup (rows <= 4: direct adds, the statistics must not move); many workgroups with the stream's scratch;
# with the scratch removed or one byte too small (atomics, one counted fallback per launch)
for _r in (1, 3, 4):
    NORM_BWD.append(NormCase(f"ln-bwd-onewg-r{_r}", _r, 764, bwd=True, dy_f32=_r != 3, opts=True))
NORM_BWD.append(NormCase("rms-bwd-onewg-r4", 4, 512, rms=True, bwd=True, dy_f32=False, opts=True))
NORM_BWD.append(NormCase("ln-bwd-r5", 5, 260, bwd=True, opts=True))
for _s in ("off", "short"):
    NORM_BWD.append(NormCase(f"ln-bwd-scratch-{_s}", 37, 768, bwd=True, dy_f32=False, opts=True, scratch=_s))
    NORM_BWD.append(NormCase(f"ln-bwd-scratch-{_s}-pred", 37, 1028, bwd=True, opts=True, scratch=_s))
    NORM_BWD.append(NormCase(f"rms-bwd-scratch-{_s}", 37, 764, rms=True, bwd=True, scratch=_s))
# the grid-stride row loop: integer dy and integer prior contents, so that dbeta is exact in every order and one row or one
# workgroup lost on a later iteration of the loop shows there (the bound of the other sums grows with the number of rows)
NORM_BWD.append(NormCase("ln-bwd-long-exact", LONG_ROWS, 768, bwd=True, dy_f32=False, opts=True, data="intdy"))
NORM_BWD.append(NormCase("ln-bwd-long-pred", LONG_ROWS, 764, bwd=True, data="intdy"))
# mixed options: dres without dx_bf16, dx_stride > width without dres, dx_colsum without branch_scale, branch_scale with dx_bf16 alone
NORM_BWD.append(NormCase("ln-bwd-mix-dres-only", 37, 764, bwd=True, mix="r"))
NORM_BWD.append(NormCase("ln-bwd-mix-stride-only", 37, 768, bwd=True, dy_f32=False, mix="s"))
NORM_BWD.append(NormCase("ln-bwd-mix-colsum-bf16", 37, 1020, bwd=True, mix="cb"))
NORM_BWD.append(NormCase("ln-bwd-mix-bscale-bf16", 37, 512, bwd=True, dy_f32=False, mix="kbs"))
NORM_BWD.append(NormCase("rms-bwd-mix-bf16-only", 37, 2044, rms=True, bwd=True, mix="b"))
for _d in ("bigmean", "const", "gamma0"):
    NORM_BWD.append(NormCase(f"ln-bwd-{_d}", 5, 764, bwd=True, data=_d, opts=True))
NORM_BWD.append(NormCase("rms-bwd-zero", 5, 260, rms=True, bwd=True, data="zero"))
NORM_BWD.append(NormCase("rms-bwd-gamma0", 5, 768, rms=True, bwd=True, data="gamma0", dy_f32=False, opts=True))

for _t in (NORM_FWD, NORM_BWD):
    _n = [c.name for c in _t]
    assert len(set(_n)) == len(_n), [n for n in _n if _n.count(n) > 1]


def norm_inputs(c, device="cpu", seed=0):
    """logical inputs of a norm case: x, gamma, beta, dy (fp32 or bf16), dres, branch_scale, and the prior contents of dgamma, dbeta,
    dx_colsum (non-zero: the sums are +=)"""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(*s, device=device, generator=g)          # noqa: E731
    R_, W = c.rows, c.width
    x = rn(R_, W)
    gamma = 1.0 + 0.5 * rn(W)
    if c.data == "bigmean":
        x = 1000.0 + 1e-2 * x
    elif c.data == "const":
        x = torch.full((R_, W), 3.25, device=device)
        x[1:] = rn(R_ - 1, W)                     # row 0 constant: variance 0
    elif c.data == "zero":
        x[0] = 0.0
    elif c.data == "gamma0":
        gamma = rn(W)
        gamma[::3] = 0.0
        gamma[1::6] *= -1.0
    d = {"x": x, "gamma": gamma, "beta": rn(W)}
    if c.bwd:
        dy = rn(R_, W)
        d["dgamma0"], d["dbeta0"] = rn(W), rn(W)
        if c.data == "intdy":
            dy = torch.randint(-4, 5, (R_, W), device=device, generator=g).float()
            d["dbeta0"] = torch.randint(-9, 10, (W,), device=device, generator=g).float()
        d["dy"] = dy if c.dy_f32 else dy.to(torch.bfloat16)
        if c.has("r"):
            d["dres"] = rn(R_, W)
        if not c.rms:
            if c.has("c"):
                d["colsum0"] = rn(W)
            if c.has("k"):
                bs = torch.tensor([0.0, 1.0, 1.0 / 0.7], device=device)
                d["branch_scale"] = bs[torch.arange(R_, device=device) % 3].float()
    return d


# ======================================================================================================================== sgemm
@dataclass
class SgemmCase:
    name: str
    path: str                 # S1 sgemm_kernel; S2..S5 sgemm128_kernel<1,1> <1,0> <0,1> <0,0>; S6 the split-K slab form
    M: int
    N: int
    K: int
    a: str = "k"              # k: A [M][lda], k contiguous;  m: A [K][lda], m contiguous;  g: general strides (m * lda + 2 k)
    b: str = "k"              # k: B [N][ldb], k contiguous;  n: B [K][ldb], n contiguous;  g: general strides (n * ldb + 3 k)
    apad: int = 0             # lda = extent + apad
    bpad: int = 0
    aoff: int = 0             # base offset of A in floats
    alpha: float = 1.0
    entry: str = "sgemm"      # sgemm | acc | splitk | splitk_acc
    cpad: int = 8             # ldc = N + cpad
    ws: str = "ok"            # split-K workspace: ok | short | misaligned

    def strides(self):
        """(sam, sak, lda, a_shape), (sbk, sbn, ldb, b_shape): element strides and the stored [rows][cols] extents"""
        M, N, K = self.M, self.N, self.K
        if self.a == "k":
            lda = K + self.apad
            A = (lda, 1, lda, (M, K))
        elif self.a == "m":
            lda = M + self.apad
            A = (1, lda, lda, (K, M))
        else:
            lda = 2 * K + self.apad
            A = (lda, 2, lda, (M, 2 * K))
        if self.b == "k":
            ldb = K + self.bpad
            B = (1, ldb, ldb, (N, K))
        elif self.b == "n":
            ldb = N + self.bpad
            B = (ldb, 1, ldb, (K, N))
        else:
            ldb = 3 * K + self.bpad
            B = (3, ldb, ldb, (N, 3 * K))
        return A, B

    def expected_path(self):
        (sam, sak, lda, _), (sbk, sbn, ldb, _) = self.strides()
        kw = dict(a_ck=sak == 1, a_cm=sam == 1, b_ck=sbk == 1, b_cn=sbn == 1, a_aligned=self.aoff % 4 == 0, b_aligned=True,
                  lda=lda, ldb=ldb)
        if self.entry.startswith("splitk") and R.splitk_splits_form(self.M, self.N, self.K, **kw):
            return "S6"
        return R.sgemm_kernel_name(self.M, self.N, self.K, **kw)


SGEMM = [
    SgemmCase("S1-K24", "S1", 70, 50, 24),
    SgemmCase("S1-K516", "S1", 33, 65, 516, alpha=-0.75),
    SgemmCase("S1-130x260", "S1", 130, 260, 32, b="n"),
    SgemmCase("S1-general-strides", "S1", 260, 516, 16, a="g", b="g"),
    SgemmCase("S1-base-off1", "S1", 260, 516, 16, aoff=1),
    SgemmCase("S1-ld-mod4", "S1", 260, 516, 16, apad=2),
    SgemmCase("S1-m-contig-odd", "S1", 261, 515, 16, a="m"),             # M % 4 != 0 with an m-contiguous A: not the 128-tile kernel
    SgemmCase("S1-acc", "S1", 70, 50, 24, entry="acc"),
    SgemmCase("S1-acc-alpha", "S1", 70, 50, 24, entry="acc", alpha=0.3),
]
for _p, _a, _b, (_M, _N) in (("S2", "k", "k", (261, 515)), ("S3", "k", "n", (261, 516)), ("S4", "m", "k", (260, 515)),
                             ("S5", "m", "n", (260, 516))):
    SGEMM += [SgemmCase(f"{_p}-odd-K16", _p, _M, _N, 16, _a, _b, apad=4, bpad=8),
              SgemmCase(f"{_p}-odd-K48", _p, _M, _N, 48, _a, _b, alpha=1.7),
              SgemmCase(f"{_p}-260x516-K16", _p, 260, 516, 16, _a, _b),
              SgemmCase(f"{_p}-260x516-K48", _p, 260, 516, 48, _a, _b, apad=8, bpad=4),
              SgemmCase(f"{_p}-acc", _p, 260, 516, 48, _a, _b, entry="acc"),
              SgemmCase(f"{_p}-acc-alpha", _p, 260, 516, 32, _a, _b, entry="acc", alpha=0.3)]
for _a, _b in (("k", "k"), ("k", "n"), ("m", "k"), ("m", "n")):
    SGEMM.append(SgemmCase(f"S6-layout-{_a}{_b}", "S6", 132, 136, 400, _a, _b, entry="splitk"))
SGEMM += [
    SgemmCase("S6-acc", "S6", 132, 136, 400, entry="splitk_acc"),
    SgemmCase("S6-alpha", "S6", 132, 136, 400, "k", "n", entry="splitk", alpha=0.3),
    SgemmCase("S6-acc-alpha", "S6", 132, 136, 400, "m", "n", entry="splitk_acc", alpha=-1.25),
    SgemmCase("S6-used-lt-splits", "S6", 132, 136, 1296, "k", "n", entry="splitk"),
    SgemmCase("S6-used-lt-splits-acc", "S6", 132, 136, 1296, "m", "k", entry="splitk_acc"),
    SgemmCase("S6-fallback-N", "S1", 132, 134, 400, entry="splitk"),
    SgemmCase("S6-fallback-K", "S1", 132, 136, 408, entry="splitk_acc", alpha=0.3),
    SgemmCase("S6-fallback-short-K", "S1", 132, 136, 240, "k", "n", entry="splitk"),
    SgemmCase("S6-fallback-big", "S2", 260, 516, 240, entry="splitk"),             # nothing to split on a 128-tile shape
    SgemmCase("S6-ws-short", "S6", 132, 136, 400, entry="splitk", ws="short"),
    SgemmCase("S6-ws-misaligned", "S6", 132, 136, 400, entry="splitk", ws="misaligned"),
]
_n = [c.name for c in SGEMM]
assert len(set(_n)) == len(_n)
# the routing boundary of launch_sgemm: M * N = 128 * 128 * 8 exactly at 256 x 512, one column less is the 64-tile kernel
BOUNDARY = (SgemmCase("boundary-above", "S2", 256, 512, 48), SgemmCase("boundary-below", "S1", 256, 511, 48))


def sgemm_inputs(c, device="cpu", seed=0):
    """-> A, B as Buf (stored layout, NaN padding) and the logical opA [M][K], opB [K][N] views"""
    g = torch.Generator(device=device).manual_seed(seed)
    (sam, sak, lda, ash), (sbk, sbn, ldb, bsh) = c.strides()
    A = Buf(ash[0], ash[1], lda, off=c.aoff, device=device)
    B = Buf(bsh[0], bsh[1], ldb, device=device)
    # general strides: the skipped elements keep the NaN pattern
    opA = A.flat[c.aoff:].as_strided((c.M, c.K), (sam, sak))
    opB = B.flat.as_strided((c.K, c.N), (sbk, sbn))
    opA.copy_(torch.randn(c.M, c.K, device=device, generator=g))
    opB.copy_(torch.randn(c.K, c.N, device=device, generator=g))
    return A, B, opA, opB


# ====================================================================================================================== InfoNCE
#              b    B     E   toff   scale
INFONCE = [(4, 5, 8, 1, 100.0), (3, 257, 24, 254, 1.0), (37, 1000, 72, 963, 100.0), (300, 300, 64, 0, 1.0),
           (272, 528, 512, 256, 1.0 / 0.07)]
DLOSS = 0.37
# (b, B, E, toff) -> the kernels of the forward, dq and d_all_p launches
INFONCE_PATHS = {(4, 5, 8, 1): ("S1", "S1", "S1"), (3, 257, 24, 254): ("S1", "S1", "S1"), (37, 1000, 72, 963): ("S1", "S1", "S1"),
                 (300, 300, 64, 0): ("S1", "S1", "S1"), (272, 528, 512, 256): ("S2", "S3", "S5")}
TIE_B, TIE_E = 600, 24
TIES = [(d, where) for d in (256, 1, 70) for where in ("first", "last", "none")]


def infonce_launch_paths(b, B, E):
    """kernels of uniir_infonce_fwd's logits and uniir_infonce_bwd's dq and d_all_p (contiguous, aligned operands)"""
    fwd = R.sgemm_kernel_name(b, B, E, True, False, True, False, lda=E, ldb=E)                 # q [b][E] . all_p [B][E]^T
    dq = R.sgemm_kernel_name(b, E, B, True, False, False, True, lda=B, ldb=E)                  # G [b][B] . all_p [B][E]
    dp = R.sgemm_kernel_name(B, E, b, False, True, False, True, lda=B, ldb=E)                  # G^T . q [b][E]
    return fwd, dq, dp


def infonce_inputs(b, B, E, device="cpu", seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    q = torch.nn.functional.normalize(torch.randn(b, E, device=device, generator=g), dim=1)
    p = torch.nn.functional.normalize(torch.randn(B, E, device=device, generator=g), dim=1)
    return q.contiguous(), p.contiguous()


def tie_inputs(delta, where, device="cpu", seed=0):
    """one query whose two equal maxima sit at j and j + delta (rows of all_p duplicated, the query equal to them), the target first,
    last or not among them -> q [1][E], all_p, toff, expected hit"""
    _, p = infonce_inputs(1, TIE_B, TIE_E, device, seed)
    t = 300
    j = {"first": t, "last": t - delta, "none": 17}[where]
    p[j + delta] = p[j]
    return p[j:j + 1].clone(), p, t, 1.0 if where == "first" else 0.0


# ================================================================================================================ hard negatives
#             b    N    I   dim
HARDNEG = [(1, 0, 0, 8), (5, 0, 4, 72), (6, 3, 0, 64), (24, 3, 7, 520), (130, 130, 129, 64)]


def hardneg_inputs(b, N, I, dim, device="cpu", seed=0):
    """rows 0 / 1 (when there are negatives): a negative that beats the positive, a negative equal to the positive (tie -> index 0)"""
    g = torch.Generator(device=device).manual_seed(seed)
    nrm = torch.nn.functional.normalize
    q = nrm(torch.randn(b, dim, device=device, generator=g), dim=1)
    p = nrm(q + 0.5 * nrm(torch.randn(b, dim, device=device, generator=g), dim=1), dim=1)
    n = nrm(torch.randn(b, max(N, 1), dim, device=device, generator=g), dim=2)[:, :N].contiguous()
    if N and b >= 2:
        n[0, N - 1] = q[0]
        n[1, 0] = p[1]
    return q.contiguous(), p.contiguous(), n


# ======================================================================================================================= softce
SOFTCE_B = 6
SOFTCE = [(n, temp, alpha) for n in (5, 256, 257, 1000) for temp in (None, 0.07) for alpha in (0.0, 0.4, 1.0)]


def softce_inputs(n, device="cpu", seed=0):
    """rows: 0 plain, 1 three positives, 2 id absent from ids_all, 3 tie for the arg-max with the positive first, 4 the same tie with
    the non-positive first, 5 plain.  -> sim, sim_m, ids_row, ids_all, expected hit of rows 3 and 4"""
    g = torch.Generator(device=device).manual_seed(seed)
    b = SOFTCE_B
    sim = 0.3 * torch.randn(b, n, device=device, generator=g)
    sim_m = 0.3 * torch.randn(b, n, device=device, generator=g)
    ids_all = torch.arange(n, device=device, dtype=torch.int64) * 3 + 100
    lo, hi = 1, n - 2                             # n = 5: 1 and 3; n >= 256: different waves
    ids_all[0] = ids_all[4] = ids_all[2]          # row 1: positives at 0, 2 and 4
    ids_row = ids_all[torch.tensor([lo, 2, 0, lo, hi, hi], device=device)].clone()
    ids_row[2] = 7                                # no such id
    sim[3, lo] = sim[3, hi] = 2.5
    sim[4, lo] = sim[4, hi] = 2.5
    return sim.contiguous(), sim_m.contiguous(), ids_row, ids_all, {3: 1.0, 4: 0.0}


# ============================================================================================================ select, fuse, pool
SELECT_DIMS = (8, 72, 768, 1100)
SELECT_ROWS, SELECT_SRC = 83, 40                 # rows not a multiple of 4; 40 source embeddings
MEANPOOL = [(3, 1, 4), (2, 3, 1028), (5, 19, 768)]
FUSE_DIMS = (8, 1028)
FUSE_TMASK = (0, 0, 1, 1, 0, 0, 1, 1, 1)         # all four mask combinations per row, nine rows
FUSE_IMASK = (0, 1, 0, 1, 0, 1, 0, 1, 1)


def fuse_inputs(dim, device="cpu"):
    g = torch.Generator(device=device).manual_seed(dim)
    n = len(FUSE_TMASK)
    txt, img = torch.randn(n, dim, device=device, generator=g), torch.randn(n, dim, device=device, generator=g)
    demb = torch.randn(n, dim, device=device, generator=g)
    return (txt, img, torch.tensor(FUSE_TMASK, dtype=torch.int64, device=device),
            torch.tensor(FUSE_IMASK, dtype=torch.int64, device=device), demb)


def select_idx(device="cpu"):
    """83 selections out of 40 embeddings: destination 5 is selected by rows 3, 4 and 73 (r, r + 1, r + 70), rows 30.. stay unselected"""
    idx = (torch.arange(SELECT_ROWS, device=device) * 7) % 30
    idx[3] = idx[4] = idx[73] = 5
    return idx.to(torch.int32)


# ==================================================================================================================== optimizer
ADAMW_COUNTS = (1, 3, 4, 1003, 1006)
ADAMW_BIG = 16384 * 256 * 4 + 5                  # the grid strides and the tail is live
ADAM = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
#              step  weight_decay  grad_scale  bf16 shadow given
ADAMW_PLAN = [(1, 0.0, 0.5, True), (2, 0.2, 0.5, False), (3, 0.2, 0.5, True), (1000, 0.2, 1.0, True)]
ADAMW_BIG_PLAN = [(2, 0.2, 0.5, True)]
EMA_COUNT, EMA_MOMENTUM = 4 * 1027, 0.995


def adamw_inputs(count, device="cpu", seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    p = torch.randn(count, device=device, generator=g)
    gr = torch.randn(count, device=device, generator=g)
    m = 0.1 * torch.randn(count, device=device, generator=g)
    v = 0.01 * torch.rand(count, device=device, generator=g)
    return p, gr, m, v
