"""tests/attention_ref.py on the CPU over the case table of the fp16 relative-bias attention (tests/attn_rel_f16_cases.py), as
tests/test_attn_general_f16_ref.py does for the fp16 general form: on each case's own data the emulator of the kernels' arithmetic in
fp16 sits inside HALF of every bound at both ends of the deferred maximum, at least one case has probabilities below 2^-14 (where the
ETA_P term carries fp16's absolute rounding), and each forward mutation that applies to this form falls outside the bound on at
least one case -- a bound that accepted them would prove nothing."""
import pytest
import torch

import attention_ref as R
from attn_rel_f16_cases import CASES, MUTATIONS, NAMES

HALF = 0.5
_cache = {}


def _prepared(c):
    """the items and their forward references (fp64), computed once per case and left unchanged"""
    if c.name not in _cache:
        _cache.clear()
        items = R.build_items(c, "cpu")
        _cache[c.name] = (items, [it.fwd_ref() for it in items])
    return _cache[c.name]


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_fp16_emulator_inside_half_the_bound(case):
    c = case
    assert c.dtype == torch.float16 and R.ETA_P[c.dtype] > 0
    items, refs = _prepared(c)
    for defer in (0.0, 0.999):
        ratios = {}
        for it, (ref, _) in zip(items, refs):
            assert it.rel_emb is not None and it.scale == 1.0
            got = it.emulate(None, None, defer=defer, with_bwd=False)
            for name, g in got.items():
                r, b = ref[name]
                assert R.compare(g, r, b) is None, (c.name, defer, name, R.compare(g, r, b))
                ratios[name] = max(ratios.get(name, 0.0), R.worst(g, r, b))
        print(f"\nOBS {c.name} defer={defer} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
        assert max(ratios.values()) <= HALF, (c.name, defer, ratios)


def test_cases_have_probabilities_below_fp16s_normal_range():
    """every size from 17 tokens up has a P below 2^-14 (the spike rows); one token has none"""
    have = {}
    for c in CASES:
        if c.tq > 700:          # (654 stands for the large sizes: the same operand recipe)
            continue
        p = torch.cat([ref[1].flatten() for ref in _prepared(c)[1]])
        have[c.name] = int(((p > 0) & (p < 2.0 ** -14)).sum())
    print("\nOBS P below 2^-14 per case:", have)
    assert all((n > 0) == (int(name.rsplit("-", 1)[1]) >= 17) for name, n in have.items()), have


def _applies(c, name):
    if name == "skip_chunk":
        return c.tq > 128
    if name in ("bias_diag_off", "drop_last_valid"):
        return c.tq > 1
    return True


@pytest.mark.parametrize("name", MUTATIONS)
def test_forward_mutation_falls_outside_the_bound(name):
    """planted in head 0 of one 16-row query tile (the first, and the last or a middle one) of every item of every case it applies
    to; rejected means that out or lse has an element outside its bound"""
    per_case = {}
    for c in CASES:
        if not _applies(c, name) or c.tq > 700:          # 1024 adds no other path for a CPU-side check of the bound
            continue
        items, refs = _prepared(c)
        applied = rejected = 0
        for it, (ref, _) in zip(items, refs):
            last = (it.Tq - 1) // 16
            for tile in sorted({0, last if name in ("drop_last_valid", "skip_chunk") else last // 2}):
                res = R.mutate(it, name, None, None, head=0, tile=tile, with_bwd=False)
                if res is None:
                    continue
                applied += 1
                rejected += any(R.compare(g, *ref[k]) is not None for k, g in res.items())
        per_case[c.name] = (rejected, applied)
    print(f"\nMUT {name}: (rejected, applied) per case {per_case}")
    assert any(a for _, a in per_case.values()), f"{name} applied to no case"
    assert any(r for r, _ in per_case.values()), f"{name} is inside the bound on every case: {per_case}"
