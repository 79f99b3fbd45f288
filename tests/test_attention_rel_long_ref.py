"""tests/attention_ref.py on the CPU over the case table of uniir_attention_rel_fwd_long / _rel_bwd_long
(tests/attention_rel_long_cases.py), as tests/test_attention_long_x_ref.py does for the general form: the emulator of the kernels'
arithmetic sits inside half of every bound at both ends of the deferred maximum, and every mutation that applies to a case is
rejected by the element-wise check.  Further, for the ground that is new here -- drel summed per key block from streamed query
chunks -- the defects planted by tests/attention_rel_long_ref.py are rejected by the drel comparison itself, while the same sums
without a defect sit inside half the bound.  (The reference's drel bound rejects all three as it stands: nothing was tightened.)"""
import pytest

import attention_ref as R
import attention_rel_long_ref as RL
import test_attention_ref as TR
from attention_rel_long_cases import CASES, NAMES


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_emulator_inside_half_the_bound(case):
    TR.test_emulator_inside_half_the_bound(case)


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_mutations_are_rejected(case):
    TR.test_mutations_are_rejected(case)


def test_the_mutations_of_the_new_ground_apply():
    for name, want in (("bias_diag_off", [c.name for c in CASES if c.tq > 1]), ("skip_chunk", [c.name for c in CASES if c.tq > 128]),
                       ("drop_shift_key", [c.name for c in CASES if c.drop_p > 0])):
        assert [c.name for c in CASES if TR._applies(c, name)] == want and len(want) >= 2, name


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_planted_drel_defects_are_rejected_by_the_drel_comparison(case):
    c = case
    items, fref, out_in, lse_in, bref = TR._prepared(c)
    m = len(items) - 1
    it, (ref, bound) = items[m], bref[m]["drel"]
    good = RL.drel_streamed(it, out_in[m], lse_in[m])
    assert R.compare(good, ref, bound) is None and R.worst(good, ref, bound) <= TR.HALF, (c.name, R.worst(good, ref, bound))
    for defect in RL.DEFECTS:
        if not RL.applies(defect, c.tq):
            continue
        for where in (0, -1):
            bad = RL.drel_streamed(it, out_in[m], lse_in[m], defect=defect, head=1, where=where)
            why = R.compare(bad, ref, bound)
            print(f"DEFECT {c.name} {defect} where={where}: {why}")
            assert why is not None, f"{c.name}: {defect} (where={where}) is inside the drel bound"
            assert R.compare(bad[:, 0], ref[:, 0], bound[:, 0]) is None, f"{c.name}: {defect} touched the other head"


def test_every_defect_applies_to_several_cases():
    for defect in RL.DEFECTS:
        assert sum(RL.applies(defect, c.tq) for c in CASES) >= 4, defect
