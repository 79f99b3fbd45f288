"""The case table of uniir_attention_fwd_long / _bwd_long (the general attention form up to 1024 x 1024 on the streaming kernels of
csrc/attention_long.hip), shared by tests/test_attention_long_x_gpu.py (the kernels against the fp64 reference) and
tests/test_attention_long_x_ref.py (the reference's own emulator and mutations on the CPU).  Not a test module.

The shapes are the smallest at which a chunk edge (128 keys; 64 queries in dK / dV, 128 in the forward and dQ), a 32-key block edge,
the 512 boundary of the resident kernels and both maxima occur; sizes far below 512 are here because every size runs the streaming
kernels.  key_len values sit on, before and behind those edges; `lens` are the packed query counts of the items (api "xlong" with
lens = uniir_attention_*_long with q_row_off, K / V dense)."""
from attention_ref import Case

PAD = 72              # extra elements of every leading dimension the caller chooses (multiple of 8)
FWD, DKDV, DQ = "attn_xlong_fwd_kernel<%d>", "attn_xlong_dkdv_kernel<%d>", "attn_xlong_dq_kernel<%d>"


def _path(drop):
    d = int(drop > 0)
    return " + ".join(k % d for k in (FWD, DKDV, DQ))


def _case(name, batch, heads, tq, tk, key_len=None, lens=None, drop_p=0.0, chained=False):
    return Case(name, _path(drop_p), "xlong", batch, heads, tq, tk, key_len=key_len, lens=lens, drop_p=drop_p, pad=PAD, chained=chained)


CASES = [
    _case("1x513-klen", 3, 2, 1, 513, key_len=(513, 512, 1)),
    _case("35x577", 3, 2, 35, 577, chained=True),
    _case("130x577-klen", 3, 2, 130, 577, key_len=(577, 576, 129)),
    _case("77x1024-klen", 3, 2, 77, 1024, key_len=(1024, 1023, 897)),
    _case("577x577-drop-klen", 2, 2, 577, 577, key_len=(577, 300), drop_p=0.1),
    _case("1024x1024", 1, 2, 1024, 1024),
    _case("rows-35x577", 5, 2, 35, 577, lens=(1, 16, 17, 23, 35)),
    _case("rows-35x577-drop-klen", 5, 2, 35, 577, lens=(1, 16, 17, 23, 35), key_len=(577, 1, 200, 512, 576), drop_p=0.1, chained=True),
    _case("rows-200x640-drop-klen", 3, 2, 200, 640, lens=(200, 1, 130), key_len=(640, 513, 128), drop_p=0.1),
    _case("35x50-drop-klen", 3, 2, 35, 50, key_len=(50, 1, 33), drop_p=0.1),
    _case("1x1", 2, 2, 1, 1),
    _case("17x128", 2, 2, 17, 128),
    _case("16x129-drop", 2, 2, 16, 129, drop_p=0.1),
]
NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)
for _c in CASES:          # the contract: no empty item, no key_len below 1
    assert _c.lens is None or (len(_c.lens) == _c.batch and min(_c.lens) >= 1 and max(_c.lens) <= _c.tq)
    assert _c.key_len is None or (len(_c.key_len) == _c.batch and min(_c.key_len) >= 1)
