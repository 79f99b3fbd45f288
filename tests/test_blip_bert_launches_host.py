"""The launch sequence of the MED BERT (blip_model.bert_forward, bert_backward) is what tests/golden/g19_bert_launches.json holds:
every ops call with all its arguments -- which parameter, gradient slice and activation buffer, which column view, which dropout seed
in which order, which keyword set -- for BLIP_FF and BLIP_SF, packed and dense rows, the last layer on all rows and on the class rows,
with and without dropout, one and two layers, forward and backward in bf16 and the forward in fp16.  The table holds a digest of
every entry (and the entries of one case in full): a mismatch prints the first entry that differs as it is now.  It was recorded
(tests/golden/make_golden_bert_launches.py) from blip_model.py as it was before the layer bodies were unified.  CPU only: the
recorder of tests/bert_launch_cases.py stands in for every op, so neither a GPU nor the library is needed."""
import json
import os

import pytest

import bert_launch_cases as K

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "g19_bert_launches.json")) as _f:
    TABLE = json.load(_f)


def test_the_table_holds_the_48_cases():
    assert len(K.CASES) == 48 and len(set(K.NAMES)) == 48 and set(TABLE["digests"]) == set(K.NAMES)
    assert sum(c["dtype"] == "bf16" for c in K.CASES) == 32
    assert set(TABLE["full"]) == set(K.FULL) <= set(K.NAMES)
    for name, entries in TABLE["full"].items():          # the entries held in full are the ones the digests stand for
        assert [K.digest(e) for e in entries] == TABLE["digests"][name].split()


@pytest.mark.parametrize("case", K.CASES, ids=K.NAMES)
def test_bert_makes_the_recorded_calls(case):
    name = K.name_of(case)
    got = json.loads(json.dumps(K.trace(case)))
    bad = K.first_difference(got, TABLE["digests"][name].split(), TABLE["full"].get(name))
    if bad is not None:
        print(bad)
    assert bad is None, bad
