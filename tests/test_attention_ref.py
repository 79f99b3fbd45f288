"""tests/attention_ref.py on the CPU: the emulator of the kernels' arithmetic sits inside every bound with room to spare, at both ends
of the deferred maximum; every mutation is rejected by the element-wise check at every shape it applies to; and the comparison
reports a wrong shape, a wrong dtype and NaN as failures.

The shapes are those of the GPU table (tests/test_attention_paths_gpu.py::CASES): of every path named there the smallest and the
largest case by tq * tk (then batch), which keeps each path's edge sizes and every feature combination; the case with more (item,
head) pairs than compute units is a property of the launch, not of the arithmetic, and is left to the GPU."""
import pytest
import torch

import attention_ref as R
from test_attention_paths_gpu import CASES

HALF = 0.5          # the emulator must stay below this fraction of every bound, so that a kernel has room


def _subset():
    by_path = {}
    for c in CASES:
        by_path.setdefault(c.path, []).append(c)
    out = []
    for cs in by_path.values():
        cs = sorted((c for c in cs if c.batch * c.heads <= 64), key=lambda c: (c.tq * c.tk, c.batch))
        for c in (cs[:1] + cs[-1:]):
            if c not in out:
                out.append(c)
    return out


SUBSET = _subset()


def _cpu_dropf(p):
    def f(count):
        g = torch.Generator().manual_seed(99)
        return (torch.rand(count, generator=g) >= p).float() / (1.0 - p)
    return f


_cache = {}


def _prepared(c):
    """items, their forward references and the backward references on the rounded reference out / lse: computed once per case"""
    if c.name not in _cache:
        _cache.clear()
        items = R.build_items(c, "cpu", _cpu_dropf(c.drop_p) if c.drop_p > 0 else None)
        fref = [it.fwd_ref()[0] for it in items]
        out_in = [f["out"][0].to(c.dtype) for f in fref]
        lse_in = [f["lse"][0].float() for f in fref]
        bref = [it.bwd_ref(o, l) if c.bwd else {} for it, o, l in zip(items, out_in, lse_in)]
        _cache[c.name] = (items, fref, out_in, lse_in, bref)
    return _cache[c.name]


def _refs(fref, bref, m):
    r = dict(fref[m])
    r.update({k: v for k, v in bref[m].items() if k != "drel_mag"})
    return r


@pytest.mark.parametrize("case", SUBSET, ids=[c.name for c in SUBSET])
def test_emulator_inside_half_the_bound(case):
    c = case
    items, fref, out_in, lse_in, bref = _prepared(c)
    for defer in (0.0, 0.999):
        ratios = {}
        for m, it in enumerate(items):
            res = it.emulate(out_in[m], lse_in[m], defer=defer, with_bwd=c.bwd)
            for name, got in res.items():
                ref, bound = _refs(fref, bref, m)[name]
                assert R.compare(got, ref, bound) is None, (c.name, m, name, R.compare(got, ref, bound))
                ratios[name] = max(ratios.get(name, 0.0), R.worst(got, ref, bound))
        print(f"\nOBS {c.name} defer={defer} " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
        assert max(ratios.values()) <= HALF, (c.name, defer, ratios)


def _applies(c, name):
    """the mutations a case must reject (mutate() returns None where one changes nothing for an item; these must apply somewhere)"""
    bwd_only = name in ("dk_scale_missing", "dk_scale_twice", "d_56_columns", "masked_key_nonzero")
    if bwd_only and not c.bwd:
        return False
    if name.startswith("causal_"):
        return c.causal and c.tq > 1
    if name in ("drop_shift_key", "lse_without_drop_correction"):
        return c.drop_p > 0 and c.tk > 1
    if name == "drop_packed_coords":
        return c.drop_p > 0 and c.lens is not None
    if name == "bias_diag_off":
        return c.api == "rel" and c.tq > 1
    if name in ("dk_scale_missing", "dk_scale_twice"):
        return c.api != "rel" and c.tk > 1
    if name == "masked_key_nonzero":
        return c.key_len is not None and any(k < c.tk for k in c.key_len)
    if name == "skip_chunk":
        return c.tk > 128
    if name == "swap_rows":
        return c.tq > 1
    if name == "drop_last_valid":
        return c.tk > 1
    if name == "admit_first_masked":
        return c.tq > 2 or (c.key_len is not None and any(k < c.tk for k in c.key_len)) or c.lens is not None
    return True


EDGE = ("admit_first_masked", "drop_last_valid", "causal_plus_one", "causal_minus_one", "skip_chunk", "masked_key_nonzero")


def _tiles(it, name):
    """the 16-row tiles a mutation is confined to, one at a time: the first, and for the mutations of the mask edge the tile of the
    item's last row (a late and often partial one: wave 0's fifth at 257 tokens, the pair kernel's odd tile), for the others a
    middle one (the last tile may hold stressed rows only, which share one query)"""
    if name in ("dk_scale_missing", "dk_scale_twice"):
        return sorted({0, ((it.kvalid - 1) // 16) // 2})
    last = (it.Tq - 1) // 16
    return sorted({0, last if name in EDGE else last // 2})


@pytest.mark.parametrize("case", SUBSET, ids=[c.name for c in SUBSET])
def test_mutations_are_rejected(case):
    c = case
    items, fref, out_in, lse_in, bref = _prepared(c)
    report = []
    for name in R.MUTATIONS:
        if not _applies(c, name):
            continue
        applied = rejected = 0
        for m, it in enumerate(items):
            for tile in _tiles(it, name):
                head = it.H - 1 if name == "drop_packed_coords" else 0          # (head 0's packed and dense coordinates can coincide)
                res = R.mutate(it, name, out_in[m], lse_in[m], head=head, tile=tile, with_bwd=c.bwd)
                if res is None:
                    continue
                applied += 1
                refs = _refs(fref, bref, m)
                bad = [k for k, got in res.items() if R.compare(got, *refs[k]) is not None]
                rejected += bool(bad)
                if not bad:
                    report.append((name, m, tile))
        assert applied, f"{c.name}: {name} applied to no item"
        print(f"MUT {c.name} {name}: rejected {rejected} of {applied}")
    assert not report, f"{c.name}: mutations inside the bound (name, item, tile): {report}"


def test_compare_reports_shape_dtype_and_nan():
    ref = torch.zeros(4, 2, 64, dtype=torch.float64)
    bound = torch.full_like(ref, 1e-3)
    ok = torch.zeros(4, 2, 64, dtype=torch.bfloat16)
    assert R.compare(ok, ref, bound, torch.bfloat16) is None
    assert "shape" in R.compare(ok[:3], ref, bound, torch.bfloat16)
    assert "shape" in R.compare(ok.reshape(4, 128), ref, bound, torch.bfloat16)
    assert "dtype" in R.compare(ok.half(), ref, bound, torch.bfloat16)
    assert "dtype" in R.compare(ok.float(), ref, bound, torch.bfloat16)
    for bad in (float("nan"), float("inf")):
        x = ok.clone()
        x[1, 1, 5] = bad
        assert "non-finite" in R.compare(x, ref, bound, torch.bfloat16)
        assert R.worst(x, ref, bound) == float("inf")
    x = ok.clone()
    x[3, 0, 0] = 0.01
    assert "outside" in R.compare(x, ref, bound, torch.bfloat16)
    assert R.compare(x, ref, torch.zeros_like(bound), torch.bfloat16) is not None          # a bound of 0 accepts exact values only
    assert R.compare(ok, ref, torch.zeros_like(bound), torch.bfloat16) is None
