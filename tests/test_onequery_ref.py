"""tests/attention_ref.py on the CPU over the case table of uniir_onequery_fwd / _bwd (tests/onequery_cases.py), and the host side of
the two entry points:
  the emulator of the kernels' arithmetic sits inside half of every bound at both ends of the deferred maximum (the one-pass backward
  rounds less often than that emulator, so the bound covers it with more room);
  the defects a one-query kernel with key counts, packed keys and dropout can have are rejected by the element-wise check: the dropout
  coordinate with a query stride of 1 instead of drop_tq, a key count off by one in either direction, the packed row base of the
  neighbouring item, the dropout factor missing from dP, non-zero dk / dv behind key_len;
  every call the entry points refuse returns its documented code and writes nothing (a refused call returns before any HIP call)."""
import ctypes as C
import math

import pytest
import torch

import attention_ref as R
from onequery_cases import CASES, NAMES, build_items

HALF = 0.5
BF = torch.bfloat16


def _cpu_dropf(p):
    def f(count):
        g = torch.Generator().manual_seed(99)
        return (torch.rand(count, generator=g) >= p).float() / (1.0 - p)
    return f


_cache = {}


def _prepared(c):
    if c.name not in _cache:
        _cache.clear()
        items = build_items(c, "cpu", _cpu_dropf(c.drop_p) if c.drop_p > 0 else None)
        fref = [it.fwd_ref()[0] for it in items]
        out_in = [f["out"][0].to(c.dtype) for f in fref]
        lse_in = [f["lse"][0].float() for f in fref]
        bref = [it.bwd_ref(o, l) for it, o, l in zip(items, out_in, lse_in)]
        _cache[c.name] = (items, fref, out_in, lse_in, bref)
    return _cache[c.name]


def _refs(fref, bref, m):
    r = dict(fref[m])
    r.update(bref[m])
    return r


def _bad(res, refs):
    return [k for k, got in res.items() if R.compare(got, *refs[k]) is not None]


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_emulator_inside_half_the_bound(case):
    c = case
    items, fref, out_in, lse_in, bref = _prepared(c)
    for defer in (0.0, 0.999):
        ratios = {}
        for m, it in enumerate(items):
            for name, got in it.emulate(out_in[m], lse_in[m], defer=defer).items():
                ref, bound = _refs(fref, bref, m)[name]
                assert R.compare(got, ref, bound) is None, (c.name, m, name, R.compare(got, ref, bound))
                ratios[name] = max(ratios.get(name, 0.0), R.worst(got, ref, bound))
        assert max(ratios.values()) <= HALF, (c.name, defer, ratios)


def _emulate(it, out_in, lse_in, *, k=None, v=None, drop="own", drop_bwd="own"):
    """the emulator on other keys / other factors -> dict like Item.emulate (drop_bwd: the factors of the backward's dP and dS)"""
    k, v = (it.k if k is None else k), (it.v if v is None else v)
    drop = it.drop if isinstance(drop, str) else drop
    o, l = R.emulate_forward(it.q, k, v, scale=it.scale, dtype=it.dtype, valid=it.valid(), drop=drop)
    dq, dk, dv, _ = R.emulate_backward(it.q, k, v, out_in, it.dout, lse_in, scale=it.scale, dtype=it.dtype, valid=it.valid(), drop=drop)
    if not isinstance(drop_bwd, str):          # dS (and with it dq, dk) from other factors than dV
        dq, dk, _, _ = R.emulate_backward(it.q, k, v, out_in, it.dout, lse_in, scale=it.scale, dtype=it.dtype, valid=it.valid(),
                                          drop=drop_bwd)
    return {"out": o, "lse": l, "dq": dq, "dk": dk, "dv": dv}


def _stride_one_factors(c, it):
    """the factors of a kernel that takes the query stride of the coordinate as 1: ((m H + h) * 1 + drop_q) tk + key"""
    H, lk = it.H, it.Tk
    h = torch.arange(H)[:, None]
    j = torch.arange(lk)[None, :]
    idx = ((it.m * H + h) + c.drop_q) * c.tk + j
    return it.drop_call[idx].reshape(H, 1, lk)


@pytest.mark.parametrize("case", CASES, ids=NAMES)
def test_planted_defects_are_rejected(case):
    c = case
    items, fref, out_in, lse_in, bref = _prepared(c)
    inside, seen = [], set()
    packed_k = torch.cat([it.k for it in items] * 2) if c.form == "packed" else None
    packed_v = torch.cat([it.v for it in items] * 2) if c.form == "packed" else None
    offs = [sum(it.Tk for it in items[:m]) for m in range(c.batch + 1)]
    stride_rejected = stride_applied = 0
    for m, it in enumerate(items):
        refs = _refs(fref, bref, m)
        # a key count off by one in either direction, non-zero dk / dv behind key_len
        for name in ("admit_first_masked", "drop_last_valid", "masked_key_nonzero"):
            res = R.mutate(it, name, out_in[m], lse_in[m], head=0, tile=0)
            if res is None:
                continue
            seen.add(name)
            if not _bad(res, refs):
                inside.append((name, m))
        if c.form == "packed":          # the rows of the neighbouring item (its base, this item's length)
            b = offs[(m + 1) % c.batch]
            res = _emulate(it, out_in[m], lse_in[m], k=packed_k[b:b + it.Tk], v=packed_v[b:b + it.Tk])
            seen.add("neighbour_base")
            if not _bad(res, refs):
                inside.append(("neighbour_base", m))
        if c.drop_p > 0:
            # the factor missing from dP: dS = p (dP - D) with D = dO . O of the dropped forward
            res = _emulate(it, out_in[m], lse_in[m], drop_bwd=None)
            seen.add("dp_without_mask")
            if not _bad(res, refs):
                inside.append(("dp_without_mask", m))
            if c.drop_tq > 1:
                wrong = _stride_one_factors(c, it)
                if not torch.equal(wrong * it.valid(), it.drop * it.valid()):
                    stride_applied += 1
                    stride_rejected += bool(_bad(_emulate(it, out_in[m], lse_in[m], drop=wrong), refs))
    assert not inside, f"{c.name}: defects inside the bound (name, item): {inside}"
    # A wrong coordinate draws other factors of the same distribution: an item shows it when a key that holds a visible share of the
    # row's probability changes its factor, which needs more than a handful of keys.  From 31 keys on every case must show it in at
    # least one of its items with more than one key; below, the count is printed.
    print(f"DEFECTS {c.name}: {sorted(seen)} stride-1 rejected {stride_rejected} of {stride_applied}")
    if c.drop_p > 0 and c.drop_tq > 1 and c.tk >= 31:
        assert stride_applied and stride_rejected, (c.name, stride_applied, stride_rejected)
    want = set()
    if c.tk > 1:
        want.add("drop_last_valid")
    if c.form != "dense" and any(c.kcount(m) < c.tk for m in range(c.batch)):
        want.add("admit_first_masked")
    if c.form == "klen" and any(c.kcount(m) < c.tk for m in range(c.batch)):
        want.add("masked_key_nonzero")
    if c.form == "packed":
        want.add("neighbour_base")
    if c.drop_p > 0:
        want.add("dp_without_mask")
    assert want <= seen, (c.name, want - seen)


# ------------------------------------------------------------------------------------------------------------------- refusals
ERR = {"OK": 0, "EINVAL": -1, "ESHAPE": -2, "EALIGN": -3}
FWD = ("q", "q_ld", "k", "v", "kv_ld", "out", "out_ld", "lse", "key_len", "kv_row_off", "batch", "tk", "heads", "drop_p", "drop_seed",
       "drop_tq", "drop_q")
BWD = ("q", "q_ld", "k", "v", "kv_ld", "out", "dout", "out_ld", "lse", "key_len", "kv_row_off", "dq", "dq_ld", "dk", "dv", "dkv_ld",
       "batch", "tk", "heads", "drop_p", "drop_seed", "drop_tq", "drop_q")
POINTERS = {"q", "k", "v", "out", "dout", "lse", "key_len", "kv_row_off", "dq", "dk", "dv"}
OPTIONAL = {"key_len", "kv_row_off"}
LDS = {"q_ld", "kv_ld", "out_ld", "dq_ld", "dkv_ld"}
ALIGNED = {"q", "k", "v", "out", "dout", "dq", "dk", "dv"}          # the pointers whose alignment is tested


def _refusal_table():
    """(entry point, what changes, {argument: value}, code): every refusal of include/uniir_hip.h, one row per argument it can come
    from; pointer values are byte offsets into the test's buffer"""
    rows = []
    for fn, names in (("uniir_onequery_fwd", FWD), ("uniir_onequery_bwd", BWD)):
        for p in names:
            if p in POINTERS and p not in OPTIONAL:
                rows.append((fn, f"{p} NULL", {p: None}, "EINVAL"))
            if p in ALIGNED:
                rows.append((fn, f"{p} + 8 bytes", {p: "+8"}, "EALIGN"))
                rows.append((fn, f"{p} + 2 bytes, tk 577", {p: "+2", "tk": 577}, "EALIGN"))
            if p in LDS:
                rows.append((fn, f"{p} + 4", {p: "+4"}, "EALIGN"))
        rows += [(fn, "heads 0", {"heads": 0}, "EINVAL"), (fn, "heads -1", {"heads": -1}, "EINVAL"),
                 (fn, "batch -1", {"batch": -1}, "EINVAL"),
                 (fn, "drop_p 1", {"drop_p": 1.0}, "EINVAL"), (fn, "drop_p -0.1", {"drop_p": -0.1}, "EINVAL"),
                 (fn, "drop_p NaN", {"drop_p": math.nan}, "EINVAL"), (fn, "drop_p NaN, batch 0", {"drop_p": math.nan, "batch": 0}, "EINVAL"),
                 (fn, "drop_tq 0", {"drop_tq": 0, "drop_q": 0}, "EINVAL"), (fn, "drop_q -1", {"drop_q": -1}, "EINVAL"),
                 (fn, "drop_q == drop_tq", {"drop_tq": 40, "drop_q": 40}, "EINVAL"),
                 (fn, "both key forms", {"key_len": "keep", "kv_row_off": "keep"}, "EINVAL"),
                 (fn, "both key forms, tk 0", {"key_len": "keep", "kv_row_off": "keep", "tk": 0}, "EINVAL"),
                 (fn, "tk 0", {"tk": 0}, "ESHAPE"), (fn, "tk 1025", {"tk": 1025}, "ESHAPE"), (fn, "tk -3", {"tk": -3}, "ESHAPE"),
                 (fn, "tk 1025 and a bad kv_ld", {"tk": 1025, "kv_ld": "+4"}, "ESHAPE"),
                 (fn, "batch 0", {"batch": 0}, "OK"), (fn, "batch 0, tk 0, q + 8 bytes", {"batch": 0, "tk": 0, "q": "+8"}, "OK")]
    return rows


REFUSALS = _refusal_table()


@pytest.mark.parametrize("fn", ["uniir_onequery_fwd", "uniir_onequery_bwd"])
def test_refused_calls_return_their_code_and_write_nothing(fn):
    from uniir_amd import _lib
    lib = _lib.load()
    names = FWD if fn.endswith("fwd") else BWD
    types = _lib.SIGNATURES[fn][1]
    assert len(types) == len(names) + 1          # + the stream
    n = 1 << 16
    raw = C.create_string_buffer(n + 256)
    base = (C.addressof(raw) + 255) & ~255
    pattern = bytes((7 * i + 3) & 255 for i in range(n))
    W = 128
    good = dict(q_ld=W, kv_ld=2 * W, out_ld=W, dq_ld=W, dkv_ld=2 * W, batch=1, tk=16, heads=2, drop_p=0.1, drop_seed=7, drop_tq=40, drop_q=39)
    for i, p in enumerate(sorted(POINTERS)):
        good[p] = 4096 * (i + 1)
    good["key_len"] = None          # one key form at most in a good call
    rows = [r for r in REFUSALS if r[0] == fn]
    assert {r[3] for r in rows} == set(ERR)
    for r in rows:          # no row may reach a launch: checked for ALL rows before the first call
        assert r[3] != "OK" or r[2].get("batch") == 0, r
    wrong = []
    for _, what, change, code in rows:
        a = dict(good)
        for k, val in change.items():
            if val == "keep":
                a[k] = 4096 * (sorted(POINTERS).index(k) + 1)
            elif isinstance(val, str):
                a[k] = good[k] + int(val)
            else:
                a[k] = val
        vals = [(None if a[p] is None else base + a[p]) if p in POINTERS else a[p] for p in names]
        C.memmove(base, pattern, n)
        rc = getattr(lib, fn)(*vals, None)
        if rc != ERR[code]:
            wrong.append((what, code, rc))
        assert C.string_at(base, n) == pattern, what
    assert not wrong, wrong


def test_the_binding_and_the_wrappers_know_the_entry_points():
    from uniir_amd import _lib, ops
    lib = _lib.load()
    for name, nargs in (("uniir_onequery_fwd", 18), ("uniir_onequery_bwd", 24)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and getattr(lib, name).argtypes is not None
        assert not name.startswith("uniir_attention_")
    assert callable(ops.onequery_fwd) and callable(ops.onequery_bwd)
