"""The case tables of tests/test_glue_paths_gpu.py, the builders of their inputs and the host arithmetic that names each case's path.

Not a test module and free of any GPU call: tests/test_glue_ref.py walks the same tables on the CPU, the GPU file runs them on the
kernels.  Builders take the device.  The host arithmetic restated here (csrc/elementwise.hip's entry points): grid_for and the grid
caps, uniir_colsum_bf16's gx / gy / rows per block, and the bucketed token gradient's kmax / nslices / scratch bytes with the
conditions under which it is refused for the atomic kernel.
"""
from dataclasses import dataclass

import numpy as np
import torch

import glue_ref as G

TOKD_SORT, TOKD_KCAP, TOKD_PER = 4096, 8, 64


# ------------------------------------------------------------------------------------------------------------------ host arithmetic
def grid_for(work, per_block=256, cap=8192):
    return max(1, min(cap, -(-work // per_block)))


# kernel -> (grid cap, work items of a launch); the work item is what one thread takes per trip of its grid-stride loop
CAPS = {
    "patchify": (16384, lambda n, g, kpad: n * g * g * (kpad // 8)),
    "vit_assemble": (16384, lambda n, T, w: n * T * (w // 4)),
    "vit_assemble_f32": (16384, lambda n, T, w: n * T * w),
    "text_embed": (16384, lambda n, ctx, w: n * ctx * (w // 4)),
    "text_embed_packed": (16384, lambda n, ctx, w: n * ctx * (w // 4)),
    "gather_rows": (8192, lambda n, w: n * (w // 4)),
    "scatter_rows": (8192, lambda n, w: n * (w // 4)),
    "act_fwd": (16384, lambda count: count // 8),
    "cast_f32_to_bf16": (16384, lambda count: count // 4 + 1),
    "cast_f32_to_f16": (16384, lambda count: count // 4 + 1),
    "cast_bf16_to_f32": (16384, lambda count: count),
    "cast_pad_rows": (8192, lambda rows, ld: rows * ld),
    "unpad_add": (8192, lambda rows, cols: rows * cols),
    "tanh_fwd": (8192, lambda count: count),
    "tanh_bwd": (8192, lambda count: count),
    "dropout_f32": (16384, lambda rows, cols: rows * (cols // 4)),
    "dropout_f32_rows": (16384, lambda rows, cols: rows * (cols // 4)),
    "dropout_bf16": (16384, lambda rows, cols: rows * (cols // 4)),
    "dropout_bf16_rows": (16384, lambda rows, cols: rows * (cols // 4)),
    "dropout_mask": (16384, lambda count: count),
}


def trips(kernel, *dims):
    """(grid, work items, trips of the busiest thread's grid-stride loop)"""
    cap, work = CAPS[kernel]
    w = work(*dims)
    g = grid_for(w, 256, cap)
    return g, w, -(-w // (g * 256))


def colsum_plan(rows, cols, out_aligned=True, scratch="on"):
    """-> dict(gx, gy, rpb, form, bytes, fallbacks): form one (a single row block adds onto the destination, no scratch asked), vec
    (stored partials, float4 reduce), col (stored partials, the one-column reduce of a misaligned destination), atomic"""
    gx = -(-cols // 512)
    gy = max(1, 2048 // gx)
    rpb = max(64, -(-rows // gy))
    gy = -(-rows // rpb)
    if gy == 1:
        return dict(gx=gx, gy=1, rpb=rpb, form="one", bytes=0, fallbacks=0)
    need = gy * cols * 4
    if scratch != "on":
        return dict(gx=gx, gy=gy, rpb=rpb, form="atomic", bytes=need, fallbacks=1)
    return dict(gx=gx, gy=gy, rpb=rpb, form="vec" if out_aligned else "col", bytes=need, fallbacks=0)


def tokd_plan(rows, vocab, w, dx_aligned=True, dtok_aligned=True, scratch="on", longest=0):
    """-> dict(form, kmax, nslices, bytes, fallbacks): form bucket (no longs table), bucket-k (kmax > 0, no id longer than
    TOKD_SORT), bucket-long, atomic.  bytes: what the launch asks the stream's scratch for (0: refused before it asks)"""
    if rows > 65535 * TOKD_SORT or vocab > 1024 * TOKD_PER or w % 4 or not dx_aligned or not dtok_aligned:
        return dict(form="atomic", kmax=0, nslices=0, bytes=0, fallbacks=1)
    kmax, nslices = rows // (TOKD_SORT + 1), -(-rows // TOKD_SORT)
    nint = (3 * vocab + 4 + rows + ((1 + kmax) if kmax else 0) + 3) & ~3
    need = (nint + (TOKD_KCAP * nslices * w if kmax else 0)) * 4
    if scratch != "on":
        return dict(form="atomic", kmax=kmax, nslices=nslices, bytes=need, fallbacks=1)
    form = "bucket" if kmax == 0 else ("bucket-long" if longest > TOKD_SORT else "bucket-k")
    return dict(form=form, kmax=kmax, nslices=nslices, bytes=need, fallbacks=0)


# ============================================================================================================== token gradient
BUCKETS = (1, 2, 3, 255, 256, 257, 4095, 4096, 4097)


@dataclass
class TokCase:
    name: str
    path: str                     # bucket | bucket-k | bucket-long | atomic
    n: int
    ctx: int
    w: int
    vocab: int
    buckets: tuple = ()           # bucket sizes that must occur exactly (ids 1 .. len, the rest of the rows get distinct ids, or id 0)
    straddle: bool = False        # the last bucket's id holds rows 4095 and 4096
    oob: bool = False             # ids below 0 and >= vocab
    dx_off: int = 0               # element offsets of the dx / dtok base pointers (1: 4 bytes off 16-byte alignment)
    dtok_off: int = 0
    scratch: str = "on"           # on | off | short

    @property
    def packed_lens(self):        # lengths of the packed form: mixed (1, ctx and in between), or full where the buckets need the rows
        return "full" if self.buckets else "mixed"

    @property
    def rows(self):
        return self.n * self.ctx


TOK = [
    TokCase("small-w4", "bucket", 5, 7, 4, 1025),
    TokCase("small-w252", "bucket", 9, 5, 252, 1023),
    TokCase("small-w256", "bucket", 9, 5, 256, 1024),
    TokCase("small-w260", "bucket", 9, 5, 260, 1025, oob=True),
    TokCase("vocab1", "bucket", 5, 7, 8, 1, oob=True),
    TokCase("vocab30524", "bucket", 16, 32, 8, 30524, oob=True),
    TokCase("vocab49408", "bucket", 8, 77, 8, 49408, oob=True),
    TokCase("vocab65536", "bucket", 8, 77, 4, 65536, oob=True),
    TokCase("rows4096", "bucket", 64, 64, 8, 1025, buckets=(1, 2, 3, 255, 256, 257)),
    TokCase("kmax-no-long", "bucket-k", 64, 65, 8, 1025, buckets=(1, 2, 3, 255, 256, 257)),
    TokCase("kmax-4095-4096", "bucket-k", 130, 77, 4, 1025, buckets=(4095, 4096)),
    TokCase("all-buckets-long", "bucket-long", 172, 77, 8, 1025, buckets=BUCKETS, straddle=True, oob=True),
    TokCase("long-w260", "bucket-long", 70, 77, 260, 1024, buckets=(257, 4097), straddle=True),
    TokCase("atomic-vocab65537", "atomic", 8, 77, 4, 65537, oob=True),
    TokCase("atomic-w6", "atomic", 9, 5, 6, 1025),
    TokCase("atomic-dx-misaligned", "atomic", 9, 5, 8, 1025, dx_off=1),
    TokCase("atomic-dtok-misaligned", "atomic", 9, 5, 8, 1025, dtok_off=1),
    TokCase("atomic-scratch-off", "atomic", 64, 65, 8, 1025, buckets=(3, 257), scratch="off"),
    TokCase("atomic-scratch-short", "atomic", 172, 77, 8, 1025, buckets=(257, 4097), scratch="short"),
]
assert len({c.name for c in TOK}) == len(TOK)


def tok_lens(c, device="cpu"):
    """packed lengths, 1 and ctx among them: drawn between 1 and ctx ("mixed"), or ctx for all items but two ("full": the cases
    whose buckets need nearly every row)"""
    g = torch.Generator().manual_seed(c.n)
    lens = torch.randint(1, c.ctx + 1, (c.n,), generator=g) if c.packed_lens == "mixed" else torch.full((c.n,), c.ctx)
    lens[0], lens[-1] = c.ctx, 1
    if c.n > 2:
        lens[1] = 1
    return lens.to(torch.int32).to(device)


def tok_text(c, device="cpu", lens=None):
    """int32 [n][ctx]: the buckets of c at ids 1 .. len(buckets) in shuffled rows, ids 0 and vocab - 1 live, the other rows spread over
    the vocabulary; with oob some rows hold ids below 0 (clamped to 0) and >= vocab (clamped to vocab - 1) -- not those of a bucket.
    With lens (the packed form) the buckets and the special ids sit in live rows, so the bucket sizes hold there too."""
    g = torch.Generator().manual_seed(c.rows * 31 + c.vocab)
    rows, V = c.rows, c.vocab
    perm = torch.randperm(rows, generator=g)
    nlive = rows
    if lens is not None:
        live = G.live_mask(lens.cpu(), c.ctx).flatten()[perm]
        perm, nlive = torch.cat([perm[live], perm[~live]]), int(live.sum())
    if c.straddle:
        perm = torch.cat([torch.tensor([4095, 4096]), perm[(perm != 4095) & (perm != 4096)]])
    text = torch.empty(rows, dtype=torch.int64)
    at = 0
    for ident, cnt in list(enumerate(c.buckets, start=1))[::-1]:      # the last bucket first: it takes perm's head (rows 4095, 4096)
        assert ident < V - 1
        text[perm[at:at + cnt]] = ident
        at += cnt
    special = [0, V - 1] + ([-1, -7, V, V + 5] if c.oob else [])
    rest = rows - at
    assert nlive - at >= len(special), (c.name, nlive, at)
    lo = len(c.buckets) + 1
    if V - 1 - lo >= rest:                   # distinct ids: buckets of one row
        fill = lo + torch.randperm(V - 1 - lo, generator=g)[:rest]
    elif V - 1 > lo:
        fill = lo + torch.randint(0, V - 1 - lo, (rest,), generator=g)
    else:
        fill = torch.zeros(rest, dtype=torch.int64)
    fill[:len(special)] = torch.tensor(special)
    text[perm[at:]] = fill
    return text.view(c.n, c.ctx).to(torch.int32).to(device)


def tok_data(c, rows, integer, device="cpu", seed=0):
    """dx [rows][w], the prior dtok [vocab][w] and dpos [ctx][w]: randn, or small integers whose absolute sum stays below 2^24"""
    g = torch.Generator().manual_seed(seed + c.w)
    if integer:
        dx = torch.randint(-4, 5, (rows, c.w), generator=g).float()
        dtok0 = torch.randint(-9, 10, (c.vocab, c.w), generator=g).float()
        dpos0 = torch.randint(-9, 10, (c.ctx, c.w), generator=g).float()
    else:
        dx, dtok0, dpos0 = torch.randn(rows, c.w, generator=g), torch.randn(c.vocab, c.w, generator=g), torch.randn(c.ctx, c.w, generator=g)
    return dx.to(device), dtok0.to(device), dpos0.to(device)


def tok_plan(c, rows, longest):
    return tokd_plan(rows, c.vocab, c.w, c.dx_off % 4 == 0, c.dtok_off % 4 == 0, c.scratch, longest)


# ======================================================================================================================== colsum
@dataclass
class ColsumCase:
    name: str
    path: str                     # one | vec | col | atomic
    rows: int
    cols: int
    pad: int = 0                  # ld = cols + pad (NaN pattern in the padding)
    out_off: int = 0              # 1: the destination 4 bytes off 16-byte alignment
    scratch: str = "on"


COLSUM = [ColsumCase(f"one-r{r}-c{c}", "one", r, c, pad=8 * (i % 2)) for i, (r, c) in
          enumerate(((1, 8), (3, 504), (4, 512), (5, 520), (63, 776), (64, 520)))]
COLSUM += [ColsumCase(f"vec-r{r}-c{c}", "vec", r, c, pad=8 * (i % 2)) for i, (r, c) in
           enumerate(((65, 8), (65, 520), (1000, 504), (1000, 512), (1000, 776)))]
COLSUM += [ColsumCase("one-misaligned", "one", 64, 520, out_off=1), ColsumCase("col-r65", "col", 65, 520, pad=8, out_off=1),
           ColsumCase("col-r1000", "col", 1000, 776, out_off=1), ColsumCase("atomic-off", "atomic", 1000, 520, pad=8, scratch="off"),
           ColsumCase("atomic-short", "atomic", 65, 776, scratch="short"),
           ColsumCase("atomic-off-misaligned", "atomic", 65, 8, out_off=1, scratch="off")]
assert len({c.name for c in COLSUM}) == len(COLSUM)


def colsum_data(c, integer, device="cpu", seed=0):
    g = torch.Generator().manual_seed(seed + c.rows + c.cols)
    if integer:
        return (torch.randint(-8, 9, (c.rows, c.cols), generator=g).to(G.BF16).to(device),
                torch.randint(-9, 10, (c.cols,), generator=g).float().to(device))
    return torch.randn(c.rows, c.cols, generator=g).to(G.BF16).to(device), torch.randn(c.cols, generator=g).to(device)


# ============================================================================================================ the exact movers
#             name          n    res  P   kpad
PATCHIFY = [("p16-g1", 2, 16, 16, 768), ("p16-g2", 3, 32, 16, 768), ("p14-k592", 2, 28, 14, 592), ("p14-k640-g16", 1, 224, 14, 640),
            ("p32-g1", 1, 32, 32, 3072), ("p32-g2-pad", 2, 64, 32, 3136)]
PATCHIFY_BIG = ("p4-strided", 43691, 16, 4, 48)
#               n   T    w
ASSEMBLE = [(1, 2, 4), (3, 2, 260), (1, 197, 768), (5, 197, 4), (2, 50, 260)]
ASSEMBLE_BIG = (2097153, 2, 4)
ASSEMBLE_F32_BIG = (524289, 2, 4)
#            n   ctx   w   vocab  oob
TEXT = [(1, 1, 4, 1, True), (3, 7, 260, 1025, True), (5, 77, 256, 49408, True), (2, 30, 252, 30524, False)]
TEXT_BIG = (1398102, 3, 4, 1000)
#             n   seq   w   idx
GATHER = [(5, 7, 4, "none"), (5, 7, 260, "item"), (9, 0, 256, "abs"), (1, 3, 8, "item"), (6, 1, 252, "none")]
GATHER_BIG = (2097155, 2, 4, "item")
CAST_COUNTS = (1, 2, 3, 4, 5, 1003)
CAST_BIG = 16384 * 256 * 4 + 4 * 50 + 3
BF16_F32_BIG = 16384 * 256 + 77
ACT_BIG = 8 * (16384 * 256 + 37)
#              rows  cols  ld
PAD_ROWS = [(1, 1, 1), (3, 5, 8), (7, 588, 592), (4, 8, 8), (5, 3, 64)]
PAD_ROWS_BIG = (262147, 3, 8)
UNPAD_BIG = (699053, 3, 8)          # rows * cols = 2097159
TANH_BIG = 8192 * 256 + 77


def gather_idx(n, seq, kind, rows_total, device="cpu"):
    """none: idx NULL; item: one offset below seq per item; abs (seq = 0): distinct absolute rows in shuffled order"""
    g = torch.Generator().manual_seed(n + seq)
    if kind == "none":
        return None
    if kind == "item":
        idx = torch.randint(0, seq, (n,), generator=g)
        idx[0], idx[-1] = seq - 1, 0
        return idx.to(torch.int32).to(device)
    return torch.randperm(rows_total, generator=g)[:n].to(torch.int32).to(device)


# ======================================================================================================================= dropout
P_TOP = 1.0 - 2.0 ** -24


@dataclass
class DropCase:
    name: str
    rows: int
    cols: int
    p: float
    outs: str = "both"            # f32 form: f32 | bf16 | both
    resid: bool = True
    div: int = 0                  # > 0: rowscale with rows_per_scale = div
    pad: int = 0                  # bf16 form: ld = cols + pad
    seed: int = 0x1234ABCD


DROP_P = (0.0, 0.1, 0.5, P_TOP, 1e-10)
DROP = [DropCase(f"p{i}", 37, 260, p, outs=("both", "f32", "bf16")[i % 3], resid=i != 2, seed=77 + i) for i, p in enumerate(DROP_P)]
DROP += [DropCase("rowscale", 37, 260, 0.1, div=5), DropCase("rowscale-bf16-out", 11, 4, 0.5, outs="bf16", div=4, resid=False),
         DropCase("pad", 37, 260, 0.1, pad=4), DropCase("pad-rowscale", 38, 8, 0.5, pad=4, div=4), DropCase("one-row", 1, 4, 0.5)]
DROP_BIG = DropCase("strided", 16384 * 256 + 5, 4, 0.1, resid=False)
DROP_MASK_BIG = 16384 * 256 + 77
assert len({c.name for c in DROP}) == len(DROP)


def drop_data(c, device="cpu"):
    g = torch.Generator().manual_seed(c.rows + c.cols)
    x, resid = torch.randn(c.rows, c.cols, generator=g), torch.randn(c.rows, c.cols, generator=g)
    nscale = -(-c.rows // c.div) if c.div else 0
    rowscale = torch.tensor([0.0, 1.0, 1.0 / 0.7], dtype=torch.float32)[torch.arange(nscale) % 3] if c.div else None
    # a strict subset of the logical rows of a tensor twice as tall, in shuffled order (the packed forms)
    row_map = torch.randperm(2 * c.rows + 3, generator=g)[:c.rows].to(torch.int32)
    mv = lambda t: None if t is None else t.to(device)          # noqa: E731
    return mv(x), mv(resid), mv(rowscale), mv(row_map)


# ================================================================================================================ pool_inv_norms
INV_NORMS = [(n, d) for n in (1, 63, 64, 65, 257) for d in (8, 64, 72, 768)]


def inv_norm_data(n, dim, device="cpu"):
    g = torch.Generator().manual_seed(n * 1000 + dim)
    x = torch.randn(n, dim, generator=g).half()
    x[n // 2] = 0.0                          # an all-zero row
    return x.to(device)


# ================================================================================================================== activations
def all_bf16(device="cpu"):
    """all 65536 bf16 bit patterns, as a bf16 tensor"""
    return torch.from_numpy(np.arange(65536, dtype=np.uint16).view(np.int16).copy()).view(G.BF16).to(device)


def tanh_data(n, device="cpu"):
    g = torch.Generator().manual_seed(n)
    x = 3.0 * torch.randn(n, generator=g)
    x[:6] = torch.tensor([0.0, 1e-30, -1e-4, 20.0, -90.0, 0.5])
    return x.to(device), torch.randn(n, generator=g).to(device)


# every path named above, for tests/test_glue_ref.py's coverage check
TOK_PATHS = {"bucket", "bucket-k", "bucket-long", "atomic"}
COLSUM_PATHS = {"one", "vec", "col", "atomic"}
