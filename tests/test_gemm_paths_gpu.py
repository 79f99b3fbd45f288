"""uniir_gemm on every dispatch path against the fp64 reference of tests/gemm_ref.py, element by element.

Each case builds a GemmDesc directly (leading dimensions, base offsets, split-K workspace, the stream's reduction scratch under
the test's control) and names the path it is meant to reach in csrc/gemm.hip:
  P1  gemm_kernel, 128 x 128 tiles          K % 64 != 0, M < 256 or N < 128
  P2  gemm_glds_kernel<.., 1>, counted loop  256 x 256 tiles with < 3 K steps in the last split, or a T-major operand whose K
                                             advance K * ld * 2 does not fit 32 bits
  P3  gemm_glds_kernel<.., 2>, ping-pong     the other 256-tile problems
  P4  gemm_glds_kernel<.., 3>                P3 with a_rowsum (bf16, both operands T-major)
  P5  gemm_glds_kernel<.., 4>                DACT, bf16, NT, one split, no bias, N / ldc / ldaux % 8, aux and C2 16-B aligned
  P6  head + tail                            ATOMIC_F32, both T-major, K % 64 != 0, K >= 1024, M >= 256, N >= 128
Every operand and output sits in a buffer with a 256-row guard band behind it, ld > its extent and optionally a leading offset;
everything outside the logical extent holds a NaN pattern.  Outputs outside [0:M, 0:N] (and the spare tails of colsum / a_rowsum)
must keep that pattern bit for bit, and NaN padding of the inputs must not reach a result.  Order-fixed sums are run twice and
compared with torch.equal."""
import ctypes as C
import re
from dataclasses import dataclass, field

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 256           # rows (and, through ld, columns) of guard band behind every tensor
COLPAD = 264          # default ld = extent + COLPAD (> 256, multiple of 8)
TAIL = 64             # spare floats behind colsum / a_rowsum
NAN16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}
NAN32 = 0x7FC00011
ERR = {"EINVAL": -1, "ESHAPE": -2, "EALIGN": -3, "EUNSUPPORTED": -5}
DT = {"bf16": torch.bfloat16, "f16": torch.float16}


@dataclass
class Case:
    name: str
    path: str
    M: int
    N: int
    K: int
    at: int = 0
    bt: int = 1
    dt: str = "bf16"
    epi: int = R.EPI_BF16
    act: int = R.ACT_QUICKGELU
    alpha: float = 1.0
    bias: bool = False
    resid: bool = False
    row_scale: bool = False
    c2: bool = False
    colsum: bool = False
    rowsum: bool = False
    splits: int = 1
    ws: str = "slab"          # slab | none | small
    pad: dict = field(default_factory=dict)     # per operand ld padding (elements): a, b, c, aux
    off: dict = field(default_factory=dict)     # per operand base offset (elements): a, b, c, aux, c2
    scratch: object = "on"    # on | off | bytes of a temporary scratch
    expect: str = "ok"        # ok or an error name
    det: bool = False         # run twice, results bitwise equal
    big: bool = False


# ----------------------------------------------------------------------------------------------------------------- the case table
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
CASES = []
_alphas = [1.0, 0.5, -3.0]
# every path x layout x 16-bit type, plain epilogue with a bias
for dt in ("bf16", "f16"):
    for i, (at, bt) in enumerate(LAYOUTS):
        al = _alphas[i % 3]
        CASES.append(Case(f"P1-{dt}-{at}{bt}", "P1", 248, 136, 72, at, bt, dt, bias=True, alpha=al))
        CASES.append(Case(f"P2-{dt}-{at}{bt}", "P2", 264, 136, 128, at, bt, dt, bias=True, alpha=al))
        CASES.append(Case(f"P3-{dt}-{at}{bt}", "P3", 520, 392, 192, at, bt, dt, bias=True, alpha=al))
# every epilogue with its optional operands, on the 128-tile and the 256-tile kernels, both 16-bit types where accepted
for dt in ("bf16", "f16"):
    for path, (M, N, K) in (("P1", (200, 136, 200)), ("P3", (520, 264, 256))):
        for act in (R.ACT_QUICKGELU, R.ACT_GELU_ERF, R.ACT_RELU):
            CASES.append(Case(f"{path}-{dt}-biasact{act}", path, M, N, K, 0, 1, dt, R.EPI_BIAS_ACT, act, bias=True, c2=True,
                              alpha=_alphas[act]))
            CASES.append(Case(f"{path}-{dt}-actonly{act}", path, M, N, K, 1, 0, dt, R.EPI_ACT_ONLY, act, bias=act != 1,
                              alpha=_alphas[act - 1]))
        CASES.append(Case(f"{path}-{dt}-f32", path, M, N, K, 0, 0, dt, R.EPI_F32, bias=True, alpha=-3.0))
        CASES.append(Case(f"{path}-{dt}-f32-nobias", path, M, N, K, 1, 1, dt, R.EPI_F32, alpha=0.5))
        CASES.append(Case(f"{path}-{dt}-resid", path, M, N, K, 0, 1, dt, R.EPI_RESID_F32, bias=True, resid=True, alpha=0.5))
        CASES.append(Case(f"{path}-{dt}-resid-scale", path, M, N, K, 1, 0, dt, R.EPI_RESID_F32, resid=True, row_scale=True))
        CASES.append(Case(f"{path}-{dt}-atomic", path, M, N, K, 1, 1, dt, R.EPI_ATOMIC_F32, alpha=-3.0))
    CASES.append(Case(f"P3-{dt}-f32-colsum", "P3", 520, 264, 256, 0, 1, dt, R.EPI_F32, bias=True, colsum=True, det=True))
for path, (M, N, K) in (("P1", (200, 136, 200)), ("P3", (520, 264, 256))):
    staged = path != "P1"
    CASES.append(Case(f"{path}-resid-c2", path, M, N, K, 0, 1, "bf16", R.EPI_RESID_F32, bias=True, resid=True, c2=True, alpha=-3.0))
    if staged:
        CASES.append(Case(f"{path}-resid-colsum", path, M, N, K, 1, 1, "bf16", R.EPI_RESID_F32, resid=True, colsum=True, det=True))
        CASES.append(Case(f"{path}-resid-all", path, M, N, K, 0, 1, "bf16", R.EPI_RESID_F32, bias=True, resid=True, row_scale=True,
                          c2=True, colsum=True, alpha=0.5, det=True))
    for act in (R.ACT_QUICKGELU, R.ACT_GELU_ERF, R.ACT_RELU):
        CASES.append(Case(f"{path}-dact{act}", path, M, N, K, 1, 0, "bf16", R.EPI_DACT, act, alpha=_alphas[act]))
        CASES.append(Case(f"{path}-dact{act}-bias", path, M, N, K, 0, 0, "bf16", R.EPI_DACT, act, bias=True))
    # DACT + C2 + colsum: the towers' c_proj dgrad (the general kernel produces C2 and the sums in separate passes and needs
    # ldaux == N for the first)
    CASES.append(Case(f"{path}-dact-c2-colsum", path, M, N, K, 0, 1 if path == "P1" else 0, "bf16", R.EPI_DACT, R.ACT_GELU_ERF,
                      c2=True, colsum=True, pad={"aux": 0}, det=staged))
# the towers' combined operands on full 256 x 256 tiles (the out_proj / c_proj forward: fast residual copy-out)
CASES.append(Case("P3-resid-all-full", "P3", 512, 512, 256, 0, 1, "bf16", R.EPI_RESID_F32, bias=True, resid=True, row_scale=True,
                  c2=True, colsum=True, det=True))
CASES.append(Case("P3-resid-full", "P3", 512, 256, 192, 0, 1, "bf16", R.EPI_RESID_F32, bias=True, resid=True))
# P5: the DACT 8-column copy-out, full and ragged tiles, with and without C2 / colsum; aux 8-B but not 16-B aligned -> P3
for act in (R.ACT_QUICKGELU, R.ACT_GELU_ERF, R.ACT_RELU):
    CASES.append(Case(f"P5-dact{act}", "P5", 512, 512, 256, 0, 1, "bf16", R.EPI_DACT, act, c2=True, colsum=True, alpha=_alphas[act],
                      det=True))
CASES.append(Case("P5-dact-ragged", "P5", 520, 264, 192, 0, 1, "bf16", R.EPI_DACT, R.ACT_QUICKGELU, c2=True, colsum=True, det=True))
CASES.append(Case("P5-dact-plain", "P5", 264, 392, 256, 0, 1, "bf16", R.EPI_DACT, R.ACT_GELU_ERF, alpha=-3.0))
CASES.append(Case("P3-dact-aux-off4", "P3", 520, 264, 192, 0, 1, "bf16", R.EPI_DACT, R.ACT_QUICKGELU, c2=True, colsum=True,
                  off={"aux": 4}, det=True))
CASES.append(Case("P1-dact-c2-aux-off4", "P1", 200, 136, 200, 0, 1, "bf16", R.EPI_DACT, R.ACT_GELU_ERF, c2=True, pad={"aux": 0},
                  off={"aux": 4}))
CASES.append(Case("P3-dact-bias", "P3", 512, 256, 192, 0, 1, "bf16", R.EPI_DACT, R.ACT_QUICKGELU, bias=True, c2=True, colsum=True))
CASES.append(Case("P2-dact", "P2", 264, 392, 128, 0, 1, "bf16", R.EPI_DACT, R.ACT_QUICKGELU, c2=True, colsum=True, det=True))
CASES.append(Case("P2-resid-all", "P2", 264, 136, 64, 0, 1, "bf16", R.EPI_RESID_F32, bias=True, resid=True, row_scale=True, c2=True,
                  colsum=True, det=True))
# boundary shapes on each side of every dispatch rule (NT, bf16 out with a bias)
for M in (8, 248, 256, 264):
    for N in (8, 120, 128, 136):
        for K in (64, 128, 192):
            big = M >= 256 and N >= 128
            path = "P1" if not big else ("P2" if K < 192 else "P3")
            CASES.append(Case(f"edge-{M}x{N}x{K}", path, M, N, K, 0, 1, "bf16", bias=True, alpha=0.5 if K == 128 else 1.0))
CASES.append(Case("ragged-2000x776x320", "P3", 2000, 776, 320, 1, 0, "bf16", R.EPI_F32))
CASES.append(Case("tiles-1056", "P3", 8320, 8064, 192, 0, 1, "bf16", bias=True))          # 33 x 32 tiles: a partial last round
# T-major / T-major weight gradients: K = 1 and 3 are the pooled-last-block wgrads at batch 1 and 3
for K in (1, 3, 8, 63, 65, 1023, 1024, 1100):
    path = "P6" if (K % 64 and K >= 1024) else ("P1" if K % 64 else ("P3" if K >= 192 else "P2"))
    CASES.append(Case(f"wgrad-K{K}", path, 256, 136, K, 1, 1, "bf16", R.EPI_ATOMIC_F32))
    CASES.append(Case(f"wgrad-K{K}-rowsum", "P4" if path == "P3" else path, 264, 256, K, 1, 1, "bf16", R.EPI_ATOMIC_F32,
                      rowsum=True, det=True))
CASES.append(Case("wgrad-K1100-f16", "P6", 256, 128, 1100, 1, 1, "f16", R.EPI_ATOMIC_F32, alpha=-3.0))
CASES.append(Case("wgrad-K2200-split4", "P6", 512, 384, 2200, 1, 1, "bf16", R.EPI_ATOMIC_F32, splits=4, rowsum=True, det=True))
# split-K: slabs, atomics (no workspace) and a workspace one float too small; 2, 3 and more splits than K steps
for splits in (2, 3, 8):
    for ws in ("slab", "none", "small"):
        det = ws == "slab"
        path = "P3" if splits != 8 else "P2"          # 8 splits of 3 K steps: 3 splits of one step each
        CASES.append(Case(f"{path}-split{splits}-{ws}", path, 264, 256, 192 * 4 if splits != 8 else 192,
                          1, 1, "bf16", R.EPI_ATOMIC_F32, splits=splits, ws=ws, det=det))
        CASES.append(Case(f"P1-split{splits}-{ws}", "P1", 200, 136, 328, 0, 1, "f16", R.EPI_ATOMIC_F32, splits=splits, ws=ws,
                          alpha=-3.0, det=det))
CASES.append(Case("P4-split3-slab", "P4", 512, 264, 1536, 1, 1, "bf16", R.EPI_ATOMIC_F32, splits=3, rowsum=True, det=True))
# strides and sub-views: bases offset by whole 16-B chunks, leading dimensions far beyond the extent; the towers' pooled wgrad
# (A at dqkv + W, lda = 3W, K = batch)
for at, bt in LAYOUTS:
    CASES.append(Case(f"view-P3-{at}{bt}", "P3", 392, 264, 256, at, bt, "bf16", R.EPI_RESID_F32, bias=True, resid=True,
                      off={"a": 8, "b": 24, "c": 16}, pad={"a": 136, "b": 72, "c": 8}))
    CASES.append(Case(f"view-P1-{at}{bt}", "P1", 136, 136, 136, at, bt, "f16", R.EPI_BF16, bias=True,
                      off={"a": 8, "b": 24, "c": 16}, pad={"a": 136, "b": 72, "c": 8}))
CASES.append(Case("tower-pooled-wgrad-b3", "P1", 256, 256, 3, 1, 1, "bf16", R.EPI_ATOMIC_F32, rowsum=True,
                  off={"a": 256}, pad={"a": 512}, det=True))
CASES.append(Case("tower-pooled-wgrad-b130", "P1", 256, 256, 130, 1, 1, "bf16", R.EPI_ATOMIC_F32, rowsum=True,
                  off={"a": 256}, pad={"a": 512}, det=True))
CASES.append(Case("tower-kv-wgrad", "P4", 512, 256, 1024, 1, 1, "bf16", R.EPI_ATOMIC_F32, splits=2, rowsum=True,
                  off={"a": 256}, pad={"a": 256}, det=True))
# colsum and a_rowsum on one descriptor: one scratch request for both; unregistered and too-small scratch keep the atomics
for epi in (R.EPI_F32, R.EPI_RESID_F32):
    for scratch in ("on", "off", 3072):           # 3072 B hold either partial region (2048 B each) but not both
        CASES.append(Case(f"P4-colsum-rowsum-{epi}-{scratch}", "P4", 512, 256, 256, 1, 1, "bf16", epi, colsum=True, rowsum=True,
                          resid=epi == R.EPI_RESID_F32, bias=True, alpha=0.5, scratch=scratch, det=scratch == "on"))
# the deterministic reductions without the stream's scratch (atomics): checked against the reference, not for bit equality
CASES.append(Case("P5-dact-noscratch", "P5", 512, 512, 256, 0, 1, "bf16", R.EPI_DACT, R.ACT_QUICKGELU, c2=True, colsum=True,
                  scratch="off"))
CASES.append(Case("P1-dact-colsum-noscratch", "P1", 2000, 136, 200, 0, 1, "bf16", R.EPI_DACT, R.ACT_QUICKGELU, colsum=True,
                  scratch="off"))
CASES.append(Case("P4-rowsum-noscratch", "P4", 512, 256, 1024, 1, 1, "bf16", R.EPI_ATOMIC_F32, splits=2, rowsum=True, scratch="off"))
# the 32-bit K advance: a T-major A of K * lda * 2 = 4 GiB must take the counted loop
CASES.append(Case("P2-k32-limit", "P2", 256, 128, 65536, 1, 0, "bf16", R.EPI_F32, pad={"a": 32768 - 256}, big=True))
# descriptors rejected by shape: nothing may be written
CASES.append(Case("reject-P1-dact-c2-ldaux", "P1", 200, 136, 200, 0, 1, "bf16", R.EPI_DACT, c2=True, expect="EUNSUPPORTED"))
CASES.append(Case("reject-P1-dact-colsum-ldc", "P1", 200, 136, 200, 0, 1, "bf16", R.EPI_DACT, colsum=True, pad={"c": 260},
                  expect="EUNSUPPORTED"))
CASES.append(Case("reject-P1-f32-colsum", "P1", 200, 136, 200, 0, 1, "bf16", R.EPI_F32, colsum=True, expect="EUNSUPPORTED"))
CASES.append(Case("reject-P1-resid-colsum", "P1", 248, 264, 256, 0, 1, "bf16", R.EPI_RESID_F32, colsum=True, expect="EUNSUPPORTED"))
for path, (M, N, K, splits) in (("P1", (200, 136, 200, 1)), ("P2", (256, 128, 64, 1)), ("P3", (256, 128, 192, 1)),
                                ("P3", (256, 128, 1024, 4)), ("P6", (256, 128, 1100, 1))):
    CASES.append(Case(f"reject-{path}-atomic-bias-s{splits}", path, M, N, K, 1, 1, "bf16", R.EPI_ATOMIC_F32, bias=True, splits=splits,
                      expect="EUNSUPPORTED"))

_names = [c.name for c in CASES]
assert len(set(_names)) == len(_names), [n for n in _names if _names.count(n) > 1]


# ------------------------------------------------------------------------------------------------------------- guarded storage
class Buf:
    """a [rows][cols] view of pitch ld at element offset off inside a flat buffer with GUARD rows behind it; every element outside
    the view holds the NaN pattern"""

    def __init__(self, rows, cols, ld, dtype, off=0):
        assert ld >= cols and ld % 4 == 0
        self.rows, self.cols, self.ld, self.off, self.dtype = rows, cols, ld, off, dtype
        n = off + (rows + GUARD) * ld
        bits = {2: torch.int16, 4: torch.int32}[dtype.itemsize]
        self.flat = torch.empty(n, dtype=dtype, device=DEV)
        self.flat.view(bits).fill_(NAN16[dtype] if dtype.itemsize == 2 else NAN32)
        self.view = self.flat[off:].as_strided((rows, cols), (ld, 1))

    def ptr(self):
        return self.view.data_ptr()

    def bits(self):
        return self.flat.view({2: torch.int16, 4: torch.int32}[self.dtype.itemsize])

    def outside_mask(self):
        m = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        m[self.off:].as_strided((self.rows, self.cols), (self.ld, 1)).fill_(False)
        return m


def _operand(rows, cols, ld, dtype, off, gen, scale=1.0):
    b = Buf(rows, cols, ld, dtype, off)
    b.view.copy_((torch.randn(rows, cols, device=DEV, generator=gen) * scale).to(dtype))
    return b


def _vec(n, gen, fill=None):
    """[n] fp32 (+ TAIL spare floats holding the NaN pattern), 256-B aligned"""
    b = Buf(1, n, n + TAIL, torch.float32)
    b.view.copy_(torch.randn(1, n, device=DEV, generator=gen) if fill is None else torch.full((1, n), fill, device=DEV))
    return b


class Run:
    """one descriptor with its buffers"""

    def __init__(self, c: Case, seed=0):
        self.c = c
        g = torch.Generator(device=DEV).manual_seed(seed)
        dt = DT[c.dt]
        M, N, K = c.M, c.N, c.K
        pad = lambda k: c.pad.get(k, COLPAD)          # noqa: E731
        off = lambda k: c.off.get(k, 0)               # noqa: E731
        sa = 1.0 / max(1.0, K ** 0.5)
        # A: [M][lda] (K contiguous) or [K][lda] (M contiguous); B: [N][ldb] or [K][ldb]
        if c.big:
            self.A = Buf(K, M, M + pad("a"), dt, 0)
            self.A.view.copy_(torch.randn(K, M, device=DEV, generator=g).to(dt))
        else:
            self.A = _operand(K, M, M + pad("a"), dt, off("a"), g) if c.at else _operand(M, K, K + pad("a"), dt, off("a"), g)
        self.B = (_operand(K, N, N + pad("b"), dt, off("b"), g, sa) if c.bt else _operand(N, K, K + pad("b"), dt, off("b"), g, sa))
        f32_out = c.epi in (R.EPI_RESID_F32, R.EPI_F32, R.EPI_ATOMIC_F32)
        self.ldc = N + pad("c")
        self.Cb = Buf(M, N, self.ldc, torch.float32 if f32_out else (dt if c.epi in (R.EPI_BF16, R.EPI_BIAS_ACT, R.EPI_ACT_ONLY)
                                                                      else torch.bfloat16), off("c"))
        self.c0 = None
        if c.epi == R.EPI_ATOMIC_F32:
            self.Cb.view.copy_(torch.randn(M, N, device=DEV, generator=g))
            self.c0 = self.Cb.view.clone()
        self.bias = _vec(N, g) if c.bias else None
        self.resid = None
        if c.resid:
            self.resid = Buf(M, N, self.ldc, torch.float32, 0)
            self.resid.view.copy_(torch.randn(M, N, device=DEV, generator=g))
        self.row_scale = None
        if c.row_scale:
            self.row_scale = _vec(M, g)
            self.row_scale.view.copy_((torch.rand(1, M, device=DEV, generator=g) < 0.7).float() / 0.7)
        self.ldaux = 0
        self.aux = None
        if c.epi == R.EPI_DACT:
            self.ldaux = N + pad("aux")
            self.aux = _operand(M, N, self.ldaux, torch.bfloat16, off("aux"), g, 2.0)
        self.C2 = None
        if c.c2:
            ld2 = self.ldaux if c.epi == R.EPI_DACT else self.ldc
            self.C2 = Buf(M, N, ld2, dt if c.epi == R.EPI_BIAS_ACT else torch.bfloat16, off("c2"))
        self.colsum = _vec(N, g) if c.colsum else None
        self.rowsum = _vec(M, g) if c.rowsum else None
        self.ws = None
        if c.splits > 1 and c.ws != "none":
            need = 4 * c.splits * M * N            # the library trims the split count to the K steps; enough for every count
            self.ws = torch.empty(need, dtype=torch.uint8, device=DEV)
            self.ws_bytes = need if c.ws == "slab" else _trimmed_splits(c) * M * N * 4 - 4

    def outputs(self):
        out = {"C": self.Cb}
        if self.C2 is not None:
            out["C2"] = self.C2
        if self.colsum is not None:
            out["colsum"] = self.colsum
        if self.rowsum is not None:
            out["rowsum"] = self.rowsum
        return out

    def desc(self):
        c = self.c
        d = _lib().GemmDesc()
        d.A, d.B, d.C = self.A.ptr(), self.B.ptr(), self.Cb.ptr()
        d.C2 = self.C2.ptr() if self.C2 is not None else None
        d.bias = self.bias.ptr() if self.bias is not None else None
        d.resid = self.resid.ptr() if self.resid is not None else None
        d.aux = self.aux.ptr() if self.aux is not None else None
        d.M, d.N, d.K = c.M, c.N, c.K
        d.lda, d.ldb, d.ldc, d.ldaux = self.A.ld, self.B.ld, self.ldc, self.ldaux
        d.a_tmaj, d.b_tmaj = c.at, c.bt
        d.epilogue, d.act, d.dtype = c.epi, c.act, 0 if c.dt == "bf16" else 1
        d.k_splits, d.alpha = c.splits, c.alpha
        if self.ws is not None:
            d.splitk_ws, d.splitk_ws_bytes = self.ws.data_ptr(), self.ws_bytes
        d.colsum = self.colsum.ptr() if self.colsum is not None else None
        d.row_scale = self.row_scale.ptr() if self.row_scale is not None else None
        d.a_rowsum = self.rowsum.ptr() if self.rowsum is not None else None
        return d

    def reference(self, got):
        c = self.c
        A = self.A.view.double()
        opA = A.t() if c.at else A
        B = self.B.view.double()
        opB = B if c.bt else B.t()
        f32_out = c.epi in (R.EPI_RESID_F32, R.EPI_F32, R.EPI_ATOMIC_F32)
        return R.gemm_reference(
            opA, opB, epilogue=c.epi, alpha=c.alpha, bias=self.bias.view[0] if self.bias is not None else None,
            resid=self.resid.view if self.resid is not None else None,
            row_scale=self.row_scale0 if self.row_scale is not None else None,
            aux=self.aux.view if self.aux is not None else None, act=c.act, c0=self.c0,
            out16=torch.float32 if f32_out else (DT[c.dt] if c.epi != R.EPI_DACT else torch.bfloat16),
            got_f=got["C"] if c.epi == R.EPI_BIAS_ACT else None,
            got_c=got["C"] if (c.epi == R.EPI_RESID_F32 and c.c2) else None,
            colsum0=self.colsum0 if self.colsum is not None else None,
            colsum_rounded=c.colsum and c.path == "P1",
            rowsum0=self.rowsum0 if self.rowsum is not None else None)


def _trimmed_splits(c):
    ksteps = -(-c.K // 64)
    s = min(c.splits, ksteps)
    per = -(-ksteps // s)
    return -(-ksteps // per)


def _lib():
    from uniir_amd import _lib
    return _lib


class _Scratch:
    """the stream's reduction scratch for one call: ops' 64 MiB buffer ("on"), none ("off") or a temporary one of `bytes`"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        from uniir_amd import ops
        self.lib = _lib().load()
        self.stream = ops._stream()            # registers ops' buffer for the current stream
        s = torch.cuda.current_stream()
        self.keep = ops._RED_SCRATCH[(s.device.index, s.cuda_stream)]
        if self.mode == "off":
            assert self.lib.uniir_reduce_scratch(None, 0, self.stream) == 0
        elif self.mode != "on":
            self.tmp = torch.empty(int(self.mode), dtype=torch.uint8, device=DEV)
            assert self.lib.uniir_reduce_scratch(C.c_void_p(self.tmp.data_ptr()), int(self.mode), self.stream) == 0
        return self.stream

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        if self.mode != "on":
            assert self.lib.uniir_reduce_scratch(C.c_void_p(self.keep.data_ptr()), self.keep.numel(), self.stream) == 0
        return False


def _call(run, scratch="on"):
    d = run.desc()
    with _Scratch(scratch) as stream:
        rc = _lib().load().uniir_gemm(C.byref(d), stream)
    return rc


def _sentinels_ok(bufs_before, run):
    for name, b in run.outputs().items():
        before = bufs_before[name]
        mask = b.outside_mask()
        if not torch.equal(b.bits()[mask], before[mask]):
            n = int((b.bits()[mask] != before[mask]).sum())
            raise AssertionError(f"{run.c.name}: {name} changed outside its extent ({n} elements)")


def _execute(c, seed=0):
    run = Run(c, seed)
    run.row_scale0 = run.row_scale.view[0].clone() if run.row_scale is not None else None
    run.colsum0 = run.colsum.view[0].clone() if run.colsum is not None else None
    run.rowsum0 = run.rowsum.view[0].clone() if run.rowsum is not None else None
    before = {k: b.bits().clone() for k, b in run.outputs().items()}
    rc = _call(run, c.scratch)
    torch.cuda.synchronize()
    return run, before, rc


@pytest.mark.parametrize("case", CASES, ids=_names)
def test_gemm_path(case):
    c = case
    run, before, rc = _execute(c)
    if c.expect != "ok":
        assert rc == ERR[c.expect], (c.name, rc)
        _sentinels_ok(before, run)
        return
    assert rc == 0, (c.name, _lib().load().uniir_strerror(rc))
    _sentinels_ok(before, run)
    got = {k: (b.view[0] if k in ("colsum", "rowsum") else b.view) for k, b in run.outputs().items()}
    ref = run.reference(got)
    for k in got:
        R.check(got[k], *ref[k], f"{c.name} ({c.path}) {k}")
    if c.det:
        run2, _, rc2 = _execute(c)
        assert rc2 == 0
        for k, b in run2.outputs().items():
            assert torch.equal(b.bits(), run.outputs()[k].bits()), f"{c.name}: {k} differs between two runs"
    del run
    if c.big:
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------- which kernel each path runs
_LOOP_OF_PATH = {"P2": 1, "P3": 2, "P4": 3, "P5": 4}          # gemm_glds_kernel<Elem, A_T, B_T, WM, WN, BK, LOOP>


def _gemm_kernels(names):
    """(kind, loop) of every GEMM main kernel among the profiler's kernel names: ("128", None) or ("256", LOOP)"""
    out = []
    for n in names:
        m = re.search(r"gemm_glds_kernel<[^>]*?(\d+)\s*>", n)
        if m:
            out.append(("256", int(m.group(1))))
        elif "gemm_kernel<" in n:
            out.append(("128", None))
    return out


def test_every_case_launches_its_paths_kernels():
    """every accepted case once more under torch.profiler: the GEMM main kernels it launches are those of the path it names"""
    from torch.profiler import ProfilerActivity, profile
    found = {}
    for c in CASES:
        if c.expect != "ok":
            continue
        run = Run(c)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            assert _call(run, c.scratch) == 0
            torch.cuda.synchronize()
        found[c.name] = (c.path, sorted({e.name.split("(")[0].replace("void ", "") for e in prof.events()
                                         if e.device_type == torch.autograd.DeviceType.CUDA}))
        del run
        if c.big:
            torch.cuda.empty_cache()
    for name, (path, kn) in found.items():
        print(f"{name:34s} {path}  {'  '.join(kn)}")
    if not any(_gemm_kernels(kn) for _, kn in found.values()):
        pytest.skip("the profiler saw none of the library's kernels")
    wrong = []
    for name, (path, kn) in found.items():
        k = _gemm_kernels(kn)
        if path == "P1":
            ok = bool(k) and all(x == ("128", None) for x in k)
        elif path == "P6":
            ok = ("128", None) in k and any(x[0] == "256" for x in k)
        else:
            ok = bool(k) and all(x == ("256", _LOOP_OF_PATH[path]) for x in k)
        if not ok:
            wrong.append((name, path, kn))
    assert not wrong, wrong
