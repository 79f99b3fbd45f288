"""tests/attention_ref.py on the CPU over the case table of the fp16 general attention form (tests/attn_general_f16_cases.py), as
tests/test_attention_ref.py does for the bf16 tables: the emulator of the kernels' arithmetic in fp16 sits inside half of every bound
at both ends of the deferred maximum, on each case's own data -- so a case can be trusted before it judges a kernel -- and the case
named WIDE has probabilities below 2^-14, where fp16's absolute rounding (the ETA_P term) is what the bound has to carry."""
import pytest
import torch

import attention_ref as R
from attn_general_f16_cases import CASES, NAMES, ONEQ, ONEQ_NAMES, WIDE, oneq_full_case

HALF = 0.5


def _inside_half(c):
    assert c.dtype == torch.float16 and R.ETA_P[c.dtype] > 0
    for it in R.build_items(c, "cpu"):
        ref = it.fwd_ref()[0]
        for defer in (0.0, 0.999):
            got = it.emulate(None, None, defer=defer, with_bwd=False)
            for name, g in got.items():
                r, b = ref[name]
                assert R.compare(g, r, b) is None, (c.name, defer, name, R.compare(g, r, b))
                assert R.worst(g, r, b) <= HALF, (c.name, defer, name, R.worst(g, r, b))


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_fp16_emulator_inside_half_the_bound(case):
    _inside_half(case)


@pytest.mark.parametrize("one", ONEQ, ids=ONEQ_NAMES)
def test_fp16_emulator_inside_half_the_bound_on_the_one_query_data(one):
    _inside_half(oneq_full_case(*one))


def test_the_wide_case_has_probabilities_below_fp16s_normal_range():
    c = CASES[NAMES.index(WIDE)]
    small = 0
    for it in R.build_items(c, "cpu"):
        p = it.fwd_ref()[1]
        small += int(((p > 0) & (p < 2.0 ** -14)).sum())
    assert small > 0
