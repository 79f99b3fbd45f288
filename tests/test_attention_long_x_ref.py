"""tests/attention_ref.py on the CPU over the case table of uniir_attention_fwd_long / _bwd_long (tests/attention_long_x_cases.py), as
tests/test_attention_ref.py does for the table of the other entry points: the emulator of the kernels' arithmetic sits inside half of
every bound at both ends of the deferred maximum, and every mutation that applies to a case is rejected by the element-wise check and
applies to at least one of its items.  All cases are taken: each is an edge of its own."""
import pytest

import attention_ref as R
import test_attention_ref as TR
from attention_long_x_cases import CASES, NAMES


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_emulator_inside_half_the_bound(case):
    TR.test_emulator_inside_half_the_bound(case)


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_mutations_are_rejected(case):
    TR.test_mutations_are_rejected(case)


def test_the_mutations_of_the_new_ground_apply():
    """what this table is for: the chunk mutation applies wherever there is more than one chunk, the packed dropout coordinates and the
    masked keys wherever the case has them"""
    for name, want in (("skip_chunk", [c.name for c in CASES if c.tk > 128]),
                       ("drop_packed_coords", [c.name for c in CASES if c.drop_p > 0 and c.lens is not None]),
                       ("masked_key_nonzero", [c.name for c in CASES if c.key_len is not None and any(k < c.tk for k in c.key_len)])):
        assert [c.name for c in CASES if TR._applies(c, name)] == want and len(want) >= 2, name
    assert set(R.MUTATIONS) >= {"skip_chunk", "drop_packed_coords", "masked_key_nonzero"}
