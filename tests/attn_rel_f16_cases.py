"""The case table of uniir_attn_rel_fwd_f16 and uniir_attn_rel_fwd_long_f16 (T5-style self-attention with the bucketed relative bias
on fp16 tensors, forward only, no dropout), shared by tests/test_attn_rel_f16_gpu.py (the kernels against the fp64 reference) and
tests/test_attn_rel_f16_ref.py (the reference's own emulator and mutations on the CPU).  Not a test module.

Resident kernel attn_fwd_kernel<1,0,1> (1 <= seq <= 512): one token, a 32-key block edge (17), the fused lengths of CLIP_FF at
ViT-B/32 (127) and ViT-L/14 (334), and the largest.  Streaming kernel attn_rlong_fwd_kernel<0,1> (1 <= seq <= 1024, every size
streams): one token, the block edge, the 128-key chunk edge (129), the first size the resident kernel refuses (513), 577 with 64
buckets (the most the entry points take), the model's own 654 = 77 + 577, and the largest.  Two items of two heads; one item at 512 and
1024.  The operands are attention_ref.build_items': the spike rows see one key at logit 27 and the others at N(0, 9), so from 17 tokens
up the unnormalised P has entries below 2^-14, where fp16 rounds absolutely (attention_ref.ETA_P).  The entry points take the packed
[q | k | v] buffer and leave no leading dimension to the caller; `pad` is carried for the machinery that reads it."""
import torch

from attention_ref import Case

F16 = torch.float16
PAD = 72
RES, LONG = "attn_fwd_kernel<1,0,1>", "attn_rlong_fwd_kernel<0,1>"
RES_FN, LONG_FN = "uniir_attn_rel_fwd_f16", "uniir_attn_rel_fwd_long_f16"


def _case(kind, seq, batch, nbuckets=32):
    tag = "res" if kind == RES else "long"
    return Case(f"rel16-{tag}-{seq}", kind, "rel", batch, 2, seq, nbuckets=nbuckets, dtype=F16, bwd=False, pad=PAD)


RESIDENT = [_case(RES, 1, 2), _case(RES, 17, 2), _case(RES, 127, 2), _case(RES, 334, 2), _case(RES, 512, 1)]
STREAMING = [_case(LONG, 1, 2), _case(LONG, 17, 2), _case(LONG, 129, 2), _case(LONG, 513, 2), _case(LONG, 577, 2, nbuckets=64),
             _case(LONG, 654, 2), _case(LONG, 1024, 1)]
CASES = RESIDENT + STREAMING
NAMES = [c.name for c in CASES]
# the forward mutations of attention_ref.mutate that apply to this form (no mask, no dropout, no backward)
MUTATIONS = ("bias_diag_off", "drop_last_valid", "row_unwritten", "head_shift", "skip_chunk")


def entry(c):
    return RES_FN if c.path == RES else LONG_FN


assert len(set(NAMES)) == len(NAMES)
for _c_ in CASES:
    assert _c_.dtype == F16 and not _c_.bwd and _c_.drop_p == 0 and _c_.tk == _c_.tq and 1 <= _c_.nbuckets <= 64
    assert _c_.tq <= (512 if _c_.path == RES else 1024)
