"""The case table of uniir_onequery_fwd / _bwd (ONE query row per item that stands for row drop_q of a call with drop_tq query rows:
per-item key counts, packed keys, dropout at the full call's coordinates), shared by tests/test_onequery_gpu.py (the kernels against
the fp64 reference and against the full calls) and tests/test_onequery_ref.py (the reference's emulator and the planted defects on
the CPU).  Not a test module.

Every case is batch 3, tq = 1, 2 heads (one case with 3: a wave of the backward's 4-head workgroup without a head).  The key
capacities sit around one load group of the backward (1, 7, 8, 9), one step of its loop (31, 32, 33) and two (64, 65), at BLIP's image
token counts (197, 577), on both sides of the forward's dispatch boundary (512, 513) and at the maximum (1024).  Every capacity runs
in three key forms -- "dense" (no key_len), "klen" (key_len over the items: 1, a middle value, tk; one case per capacity class also
holds a value above tk) and "packed" (kv_row_off, lengths 1, middle, tk) -- each without and with dropout (0.1).  The dropout
coordinate (drop_tq, drop_q) alternates between (1, 0), (40, 39) and (40, 0) -- (40, 0) is what BLIP's class row passes -- the layout
between "qkv" (k / v the K and V thirds of a [q | k | v] buffer, dk / dv the same thirds of a gradient buffer; with dense keys q is row
m * tk of that buffer, q_ld = tk * 3 W, and dq the same row of the gradient buffer: nothing is copied) and "split" (k | v in a buffer of
their own, every leading dimension padded by PAD)."""
from dataclasses import dataclass

import torch

import attention_ref as R

PAD = 72
BATCH = 3
CAPS = (1, 7, 8, 9, 31, 32, 33, 64, 65, 197, 512, 513, 577, 1024)
FORMS = ("dense", "klen", "packed")
COORDS = ((1, 0), (40, 39), (40, 0))
FULL_TQ = 40          # the query count of the full calls the forward is compared with


@dataclass
class OneCase:
    name: str
    path: str
    form: str                     # "dense" | "klen" | "packed"
    heads: int
    tk: int
    lens: tuple                   # per item: key_len ("klen", may exceed tk) or the packed length; None for "dense"
    drop_p: float
    drop_tq: int
    drop_q: int
    layout: str                   # "qkv" | "split"
    seed: int
    batch: int = BATCH
    tq: int = 1
    dtype: torch.dtype = torch.bfloat16
    bwd: bool = True
    pad: int = PAD

    def kcount(self, m):
        """the keys item m attends to"""
        return self.tk if self.lens is None else min(self.lens[m], self.tk)


def _lens(form, tk, n):
    mid = max(1, tk // 2 + 1) if tk > 2 else 1
    if form == "dense":
        return None
    if form == "klen":
        return ((1, mid, tk), (tk + 5, 1, mid), (mid, tk, tk + 1))[n % 3]          # two of three rotations hold a value above tk
    return ((1, mid, tk), (tk, 1, mid), (mid, tk, 1))[n % 3]


CASES = []


def _case(tk, form, drop_p, heads=2):
    n = len(CASES)
    ci, fi = (CAPS.index(tk) + heads) % len(CAPS), FORMS.index(form)
    drop_tq, drop_q = COORDS[(ci + fi + (drop_p > 0)) % 3]
    layout = ("qkv", "split")[(ci + fi) % 2]
    fwd = "attn_fwd_kernel<0,%d,0> (tq = 1)" % (drop_p > 0) if tk <= 512 else "attn_xlong_fwd_kernel<%d> (tq = 1)" % (drop_p > 0)
    plain = form == "dense" and drop_p == 0
    bwd = "attn_one_bwd_kernel" if plain else "attn_onex_bwd_kernel<%d>" % (drop_p > 0)
    name = f"1x{tk}-h{heads}-{form}-drop{int(drop_p * 10)}-tq{drop_tq}q{drop_q}-{layout}"
    CASES.append(OneCase(name, f"{fwd} + {bwd}", form, heads, tk, _lens(form, tk, n), drop_p, drop_tq, drop_q, layout, seed=n))


for _tk in CAPS:
    for _form in FORMS:
        for _p in (0.0, 0.1):
            _case(_tk, _form, _p)
for _form in FORMS:
    _case(577, _form, 0.1, heads=3)

NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)
for _form in FORMS:          # every key form meets every coordinate pair and both layouts, with and without dropout
    for _p in (0.0, 0.1):
        _cs = [c for c in CASES if c.form == _form and c.drop_p == _p]
        assert {(c.drop_tq, c.drop_q) for c in _cs} == set(COORDS) and {c.layout for c in _cs} == {"qkv", "split"}, (_form, _p)
assert any(c.form == "klen" and max(c.lens) > c.tk for c in CASES)


def build_items(c, device, dropf=None):
    """the items of a case -> list of attention_ref.Item (tq = 1; k / v are the item's own rows: tk dense rows, or its packed length).
    Every item carries `twin`: q [FULL_TQ][H][64] whose row drop_q is the item's query when drop_tq == FULL_TQ (the other rows are
    other data) and k / v of the full tk rows -- behind a packed item's length they hold values that would take over the row if they
    were read.  dropf(count) -> count dropout factors (fp32, flat) of the full call's dense coordinates."""
    gen = torch.Generator(device=device).manual_seed(5000 + c.seed)
    H = c.heads
    drop_all = None
    if c.drop_p > 0:
        drop_all = dropf(c.batch * H * c.drop_tq * c.tk).reshape(c.batch, H, c.drop_tq, c.tk)
    items = []
    for m in range(c.batch):
        kc = c.kcount(m)
        q, k, v, do, srows = R._operands(1, c.tk, H, c.dtype, gen, key_len=None if c.lens is None else kc, device=device)
        lk = kc if c.form == "packed" else c.tk
        it = R.Item(q, k[:lk], v[:lk], do, 0.125, c.dtype, key_len=(c.lens[m] if c.form == "klen" else None),
                    drop=None if drop_all is None else drop_all[m, :, c.drop_q:c.drop_q + 1, :lk],
                    drop_dense=None if drop_all is None else drop_all[m].flatten(), dense_tq=c.drop_tq, dense_tk=c.tk,
                    behind_k=k[lk] if lk < c.tk else None, behind_v=v[lk] if lk < c.tk else None)
        qfull = torch.randn(FULL_TQ, H, R.D, generator=gen, device=device).to(c.dtype)
        if c.drop_tq == FULL_TQ:
            qfull[c.drop_q] = q[0]
        it.twin = (qfull, k, v, do)
        it.stressed = srows
        it.m = m
        it.drop_call = None if drop_all is None else drop_all.flatten()          # the whole call's factors, from coordinate 0
        items.append(it)
    return items
