"""The case table of uniir_attn_general_fwd_f16 and uniir_onequery_fwd_f16 (tests/test_attn_general_f16_gpu.py runs it on the device,
tests/test_attn_general_f16_ref.py checks on the CPU that correct fp16 arithmetic fits the bound on each case's data).

Not a test module.  The operands are those of the f16-* and long-f16-* cases of tests/test_attention_paths_gpu.py
(attention_ref.build_items: rows that stress the mask edge, masked positions that would dominate, an early and a late spike); the
spike rows see one key at logit 27 and the others at N(0, 9), so in every case with at least 8 valid keys the unnormalised P of those
rows has entries far below 2^-14, the range where fp16 rounds absolutely (attention_ref.ETA_P); WIDE names the case the CPU test
asserts it on.

Sizes: the kernels' edges.  Resident kernel (max(tq, tk) <= 512): 32-key blocks, 16-row query tiles over 8 waves, the staging
instantiations at Tkp <= 128 / <= 320 / above.  Streaming kernel (above 512): 128 query rows per workgroup (129 x 513: the second
workgroup holds one row; packed lengths {1, 130, 64}: the third item's second workgroup leaves early), K / V in 128-key chunks (513:
one key in the fifth chunk, 577, 640: a whole last chunk, 1024: the largest), key_len on, before and behind chunk edges."""
import torch

from attention_ref import Case

F16 = torch.float16
PAD = 72              # extra elements of every leading dimension the caller chooses (multiple of 8)
RES, XL = "attn_fwd_kernel<0,0,1>", "attn_xlong_fwd_kernel<0,1>"


def _c(name, path, batch, heads, tq, tk, key_len=None, lens=None, kv_packed=0):
    return Case(name, path, "gen16", batch, heads, tq, tk, key_len=key_len, lens=lens, kv_packed=kv_packed, dtype=F16, bwd=False, pad=PAD)


CASES = [
    # resident, dense
    _c("res-1x1", RES, 2, 2, 1, 1),
    _c("res-5x33", RES, 3, 3, 5, 33),
    _c("res-16x32", RES, 2, 2, 16, 32),
    _c("res-17x31", RES, 2, 3, 17, 31),
    _c("res-30x197-klen", RES + " key_len", 3, 2, 30, 197, key_len=(1, 33, 197)),
    _c("res-512x512-klen", RES + " key_len", 3, 2, 512, 512, key_len=(512, 1, 257)),
    # packed query rows
    _c("rows-kv0-20x40", RES + " q_row_off, row_off_q_only", 3, 2, 20, 40, key_len=(40, 1, 33), lens=(1, 20, 7)),
    _c("rows-kv1-33", RES + " q_row_off", 3, 3, 33, 33, lens=(1, 33, 16), kv_packed=1),
    # streaming, dense
    _c("xl-1x513", XL, 2, 2, 1, 513),
    _c("xl-30x577", XL, 2, 3, 30, 577),
    _c("xl-30x640", XL, 2, 2, 30, 640),
    _c("xl-129x513", XL, 2, 2, 129, 513),
    _c("xl-16x1024", XL, 2, 2, 16, 1024),
    # streaming, key_len
    _c("xl-klen-577-a", XL + " key_len", 3, 2, 20, 577, key_len=(1, 128, 129)),
    _c("xl-klen-577-b", XL + " key_len", 3, 2, 20, 577, key_len=(512, 513, 577)),
    # streaming, packed query rows
    _c("xl-rows-130x577", XL + " q_row_off key_len", 3, 2, 130, 577, key_len=(577, 129, 513), lens=(1, 130, 64)),
]
NAMES = [c.name for c in CASES]
WIDE = "xl-30x577"

# the one-query form: (name, tk, key form, per-item key counts); the full call it is row 0 of has FULL_TQ query rows
FULL_TQ = 3
ONEQ = [
    ("one-klen-197", 197, "klen", (1, 33, 197)),
    ("one-klen-577", 577, "klen", (129, 577, 512)),
    ("one-packed-512", 512, "packed", (1, 512, 300)),
    ("one-packed-577", 577, "packed", (1, 577, 300)),
]
ONEQ_NAMES = [o[0] for o in ONEQ]


def oneq_full_case(name, tk, form, counts):
    """the full call a one-query case is row 0 of.  Dense keys: FULL_TQ x tk with key_len.  Packed keys up to 512: the packed
    self-attention form (kv_packed = 1, tq = tk, lens = the counts); above 512 the library has no fully packed form, so the full call
    is the dense one with key_len = the counts -- the streaming kernel never stages a masked key, so a packed item's sweep is the
    dense item's."""
    if form == "packed" and tk <= 512:
        return _c(name, RES + " (tq = 1)", len(counts), 2, tk, tk, lens=counts, kv_packed=1)
    return _c(name, (RES if tk <= 512 else XL) + " (tq = 1)", len(counts), 2, FULL_TQ, tk, key_len=counts)


assert len(set(NAMES)) == len(NAMES) and WIDE in NAMES
for _c_ in CASES:          # the contract: no empty item, no key_len below 1; heads 2 - 3, batch 2 - 3
    assert _c_.lens is None or min(_c_.lens) >= 1
    assert _c_.key_len is None or min(_c_.key_len) >= 1
    assert 2 <= _c_.heads <= 3 and 2 <= _c_.batch <= 3
    assert (max(_c_.tq, _c_.tk) > 512) == _c_.path.startswith(XL)
