"""The case table of uniir_attention_rel_fwd_long / _rel_bwd_long (T5-style self-attention with the bucketed relative bias on the
streaming kernels attn_rlong_* of csrc/attention_long.hip, 1 <= seq <= 1024), shared by tests/test_attention_rel_long_gpu.py (the
kernels against the fp64 reference) and tests/test_attention_rel_long_ref.py (the reference's own emulator and mutations on the CPU).
Not a test module.

The shapes are the smallest at which each of these occurs: one token, a 32-key block edge (17), a 128-key chunk edge and a 64-query
chunk edge (129), the 512 boundary of the resident kernels (513), the vision tower's 577 (64 buckets: the most the entry points
take), the model's own 654 = 77 + 577 (three items; once chained, once with dropout), and the maximum.  Every size runs the streaming
kernels, so sizes far below 512 belong here.  The entry points take the packed [q | k | v] buffer and leave no leading dimension to
the caller; `pad` is carried as in the x-long table for the machinery that reads it."""
from attention_ref import Case

PAD = 72
FWD, DKDV, DQ = "attn_rlong_fwd_kernel<%d>", "attn_rlong_dkdv_kernel<%d>", "attn_rlong_dq_kernel<%d>"


def _path(drop):
    d = int(drop > 0)
    return " + ".join(k % d for k in (FWD, DKDV, DQ))


def _case(seq, batch, drop_p=0.0, nbuckets=32, chained=False, tag=""):
    return Case(f"rel-long-{seq}{tag}", _path(drop_p), "rel", batch, 2, seq, drop_p=drop_p, nbuckets=nbuckets, pad=PAD, chained=chained)


CASES = [
    _case(1, 2),
    _case(17, 2, drop_p=0.1, tag="-drop"),
    _case(129, 2, drop_p=0.1, tag="-drop"),
    _case(513, 2),
    _case(577, 2, drop_p=0.1, nbuckets=64, tag="-drop-64"),
    _case(654, 3, chained=True),
    _case(654, 2, drop_p=0.1, tag="-drop"),
    _case(1024, 1),
]
NAMES = [c.name for c in CASES]
assert len(set(NAMES)) == len(NAMES)
