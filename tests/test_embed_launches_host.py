"""The launch sequences of the embedding forwards are what tests/golden/g20_embed_launches.json holds: every ops call with all its
arguments -- which parameter of the store, which temporary, which column view, which scalar -- of the fp32 forwards of CLIP, CLIP_FF
(towers without pooling and the T5 stack), the BLIP ViT, the MED BERT and BLIP_SF, and of the 16-bit forward-only passes in bf16 and
fp16.  The table holds a digest of every entry (and the entries of one case in full): a mismatch prints the first entry that differs
as it is now.  It was recorded (tests/golden/make_golden_embed_launches.py) before the fp32 launch layer and the precision rule were
each made one.  One later edit: the fp16 cases that read the padded patch weight (fp16-vit, fp16-clipff-vision, fp16-sf) lost the entry
of the store's first-use fp16 cast -- the padded fp16 copy is the store's now and is made with that cast (FlatStore.half_shadow), which
a model does before its forward and the cases do before their trace; tests/test_half_shadow_host.py pins those calls.  CPU only: the recorder of tests/bert_launch_cases.py stands in for every op, so neither a GPU nor the library is
needed."""
import json
import os

import pytest

import embed_launch_cases as E

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "g20_embed_launches.json")) as _f:
    TABLE = json.load(_f)


def test_the_table_holds_the_20_cases_and_only_the_clip_tower_fp32_cases_are_loose():
    assert len(E.NAMES) == 20 and len(set(E.NAMES)) == 20 and set(TABLE["digests"]) == set(E.NAMES)
    assert sum(n.startswith("fp32-") for n in E.NAMES) == 10 and sum(n.startswith("fp16-") for n in E.NAMES) == 5
    # the temporaries' numbers are blanked only where the shared pre-LN body had to pick one convention: the CLIP towers in fp32
    assert tuple(TABLE["loose"]) == E.LOOSE and set(E.LOOSE) <= {n for n in E.NAMES if n.startswith("fp32-clip")}
    assert set(TABLE["full"]) == set(E.FULL) <= set(E.NAMES) - set(E.LOOSE)
    for name, entries in TABLE["full"].items():          # the entries held in full are the ones the digests stand for
        assert [E.digest(e) for e in entries] == TABLE["digests"][name].split()
        assert any("@#" in json.dumps(e) for e in entries)


@pytest.mark.parametrize("name", E.NAMES)
def test_the_forward_makes_the_recorded_calls(name):
    got = E.normalised(name, E.trace(name))
    assert ("@#0" in json.dumps(got)) == (name not in E.LOOSE)          # a strict case keeps the numbers of its temporaries
    bad = E.first_difference(got, TABLE["digests"][name].split(), TABLE["full"].get(name))
    if bad is not None:
        print(bad)
    assert bad is None, bad
