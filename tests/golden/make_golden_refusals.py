#!/usr/bin/env python
"""Generates tests/golden/g17_attention_refusals.json: what the 17 attention entry points of libuniir_hip.so answer to calls they
refuse, recorded from a build of the library (the commit BEFORE a change of the host layer: the table then pins that change).

Run:  python tests/golden/make_golden_refusals.py --commit <hash of the recorded build> [--lib path/to/libuniir_hip.so]
      (CPU only: a refused call returns before any HIP call, so the library needs no GPU for this)

Every entry point gets its refusal branches IN SOURCE ORDER (CHECKS below): one row per variant of a branch, and one row per pair of
neighbouring branches failing together, which pins which check wins.  EXTRA holds the differences between entry points that are
intended (include/uniir_hip.h): where drop_p is tested relative to batch == 0, which pointers are tested for
alignment, which code a bad kv_ld gets.

Pointers are addresses inside ONE host buffer ("p:<offset>": 256-byte aligned slots, +2 for a misaligned one; null = NULL).  No row
may reach a launch: a row is only written when its code is non-zero or its batch is 0, and never with UNIIR_ELAUNCH (a launch that
was tried).  tests/test_attention_refusals_host.py replays the table: equal codes, and the buffer byte-for-byte untouched.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from uniir_amd import _lib  # noqa: E402

BUF_BYTES = 16384
ELAUNCH = -4
BIG = 2 ** 31 - 1            # a batch whose grid no longer fits 31 bits (the streaming launchers answer UNIIR_ESHAPE before they launch)

PACKED_F = ["qkv", "out", "lse"]
PACKED_B = ["qkv", "out", "dout", "lse", "dqkv"]
SEP_F = ["q", "q_ld", "k", "v", "kv_ld", "out", "out_ld", "lse"]
SEP_B = ["q", "q_ld", "k", "v", "kv_ld", "out", "dout", "out_ld", "lse"]
GRADS = ["dq", "dq_ld", "dk", "dv", "dkv_ld"]
DROP = ["drop_p", "drop_seed", "stream"]
REL = ["rel_emb", "rel_bucket", "nbuckets", "scale"]
ARGS = {
    "uniir_attention_fwd": PACKED_F + ["batch", "seq", "heads", "causal", "stream"],
    "uniir_attention_bwd": PACKED_B + ["batch", "seq", "heads", "causal", "stream"],
    "uniir_attention_fwd_packed": PACKED_F + ["row_off", "batch", "seq", "heads", "causal", "stream"],
    "uniir_attention_fwd_f16": PACKED_F + ["row_off", "batch", "seq", "heads", "causal", "stream"],
    "uniir_attention_bwd_packed": PACKED_B + ["row_off", "batch", "seq", "heads", "causal", "stream"],
    "uniir_attention_fwd_ex": SEP_F + ["key_len", "batch", "tq", "tk", "heads", "causal"] + DROP,
    "uniir_attention_bwd_ex": SEP_B + ["key_len"] + GRADS + ["batch", "tq", "tk", "heads", "causal"] + DROP,
    "uniir_attention_fwd_rows": SEP_F + ["q_row_off", "kv_packed", "key_len", "batch", "tq", "tk", "heads"] + DROP,
    "uniir_attention_bwd_rows": SEP_B + ["q_row_off", "kv_packed", "key_len"] + GRADS + ["batch", "tq", "tk", "heads"] + DROP,
    "uniir_attention_fwd_long": SEP_F + ["q_row_off", "key_len", "batch", "tq", "tk", "heads"] + DROP,
    "uniir_attention_bwd_long": SEP_B + ["q_row_off", "key_len"] + GRADS + ["batch", "tq", "tk", "heads"] + DROP,
    "uniir_attention_one_fwd": ["q", "k", "v", "kv_ld", "out", "lse", "batch", "tk", "heads", "f16", "stream"],
    "uniir_attention_one_bwd": ["q", "k", "v", "kv_ld", "out", "dout", "lse"] + GRADS + ["batch", "tk", "heads", "stream"],
    "uniir_attention_rel_fwd": PACKED_F + REL + ["batch", "seq", "heads"] + DROP,
    "uniir_attention_rel_bwd": PACKED_B + REL + ["drel", "batch", "seq", "heads"] + DROP,
    "uniir_attention_rel_fwd_long": PACKED_F + REL + ["batch", "seq", "heads"] + DROP,
    "uniir_attention_rel_bwd_long": PACKED_B + REL + ["drel", "batch", "seq", "heads"] + DROP,
}
# a call that every entry point would accept (and launch): the rows below change it
GOOD = {"batch": 2, "seq": 8, "tq": 8, "tk": 8, "heads": 2, "causal": 0, "q_ld": 128, "kv_ld": 256, "out_ld": 128, "dq_ld": 128,
        "dkv_ld": 256, "nbuckets": 32, "scale": 1.0, "drop_p": 0.0, "drop_seed": 1, "kv_packed": 0, "f16": 0}
NULL_BY_DEFAULT = {"stream", "key_len"}          # optional pointers; row_off / q_row_off: NULL where the entry point allows it
OPTIONAL_ROW_OFF = {"uniir_attention_fwd_f16", "uniir_attention_fwd_long", "uniir_attention_bwd_long"}
MIS, PTR = "misaligned", "pointer"


def null(*names):
    return [{n: None} for n in names]


def mis(*names):
    return [{n: MIS} for n in names]


def basics(ptrs, more=()):
    return null(*ptrs) + [{"batch": -1}, {"heads": 0}] + list(more)


BATCH0 = [{"batch": 0}]
BAD_DROP = [{"drop_p": 1.5}, {"drop_p": 1.0}, {"drop_p": -0.125}]
BAD_DROP_NAN = BAD_DROP + [{"drop_p": "nan"}]
LD3 = [{"q_ld": 132}, {"kv_ld": 260}, {"out_ld": 132}]
LD5 = LD3 + [{"dq_ld": 132}, {"dkv_ld": 260}]
NB = [{"nbuckets": 0}, {"nbuckets": 65}]


def shape2(mx):
    return [{"tq": 0}, {"tk": 0}, {"tq": mx + 1}, {"tk": mx + 1}]


def grid(**kw):          # only the streaming launchers test the grid: a size they run, and more workgroups than 31 bits hold
    return [{"batch": BIG, "heads": 2, **kw}]


# entry point -> its refusal branches in source order; a branch = the variants that take it
CHECKS = {
    "uniir_attention_fwd": [basics(PACKED_F), BATCH0, [{"seq": 0}, {"seq": 1025}, {"seq": 513, "causal": 1}], mis("qkv", "out"),
                            grid(seq=513)],
    "uniir_attention_bwd": [basics(PACKED_B), BATCH0, [{"seq": 0}, {"seq": 1025}, {"seq": 513, "causal": 1}],
                            mis("qkv", "out", "dout", "dqkv"), grid(seq=513)],
    "uniir_attention_fwd_packed": [basics(PACKED_F + ["row_off"]), BATCH0, [{"seq": 0}, {"seq": 513}], mis("qkv", "out")],
    "uniir_attention_fwd_f16": [basics(PACKED_F), BATCH0,
                                [{"seq": 0}, {"seq": 1025}, {"seq": 513, "causal": 1}, {"seq": 513, "row_off": PTR}],
                                mis("qkv", "out"), grid(seq=513)],
    "uniir_attention_bwd_packed": [basics(PACKED_B + ["row_off"]), BATCH0, [{"seq": 0}, {"seq": 513}],
                                   mis("qkv", "out", "dout", "dqkv")],
    "uniir_attention_fwd_ex": [basics(["q", "k", "v", "out", "lse"]), BATCH0, shape2(512), [{"causal": 1, "tk": 7}], LD3,
                               mis("q", "k", "v", "out"), BAD_DROP],
    "uniir_attention_bwd_ex": [basics(["q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv"]), BATCH0, shape2(512),
                               [{"causal": 1, "tk": 7}], LD5, mis("dq", "dk", "dv"), BAD_DROP],
    "uniir_attention_fwd_rows": [basics(["q", "k", "v", "out", "lse", "q_row_off"]), BATCH0, shape2(512),
                                 [{"kv_packed": 1, "tk": 7}, {"kv_packed": 1, "key_len": PTR}], LD3, mis("q", "k", "v", "out"),
                                 BAD_DROP],
    "uniir_attention_bwd_rows": [basics(["q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv", "q_row_off"]), BATCH0, shape2(512),
                                 [{"kv_packed": 1, "tk": 7}, {"kv_packed": 1, "key_len": PTR}], LD5, mis("dq", "dk", "dv"), BAD_DROP],
    "uniir_attention_fwd_long": [basics(["q", "k", "v", "out", "lse"]), BAD_DROP_NAN, BATCH0, shape2(1024), LD3,
                                 mis("q", "k", "v", "out"), grid(tq=600)],
    "uniir_attention_bwd_long": [basics(["q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv"]), BAD_DROP_NAN, BATCH0, shape2(1024),
                                 LD5, mis("q", "k", "v", "out", "dout", "dq", "dk", "dv"), grid(tk=600)],
    "uniir_attention_one_fwd": [basics(["q", "k", "v", "out", "lse"]), BATCH0, [{"tk": 0}, {"tk": 1025}], [{"kv_ld": 260}],
                                mis("q", "k", "v", "out"), grid(tk=513)],
    "uniir_attention_one_bwd": [basics(["q", "k", "v", "out", "dout", "lse", "dq", "dk", "dv"]), BATCH0, [{"tk": 0}, {"tk": 1025}],
                                [{"kv_ld": 260}, {"dq_ld": 132}, {"dkv_ld": 260}],
                                mis("q", "k", "v", "out", "dout", "dq", "dk", "dv"), grid(heads=8)],
    "uniir_attention_rel_fwd": [basics(PACKED_F + ["rel_emb", "rel_bucket"], NB), BATCH0, [{"seq": 0}, {"seq": 513}], BAD_DROP],
    "uniir_attention_rel_bwd": [basics(PACKED_B + ["rel_emb", "rel_bucket"], NB), BATCH0, [{"seq": 0}, {"seq": 513}], BAD_DROP],
    "uniir_attention_rel_fwd_long": [basics(PACKED_F + ["rel_emb", "rel_bucket"], NB), BAD_DROP_NAN, BATCH0,
                                     [{"seq": 0}, {"seq": 1025}], mis("qkv", "out"), grid(seq=600)],
    "uniir_attention_rel_bwd_long": [basics(PACKED_B + ["rel_emb", "rel_bucket"], NB), BAD_DROP_NAN, BATCH0,
                                     [{"seq": 0}, {"seq": 1025}], mis("qkv", "out", "dout", "dqkv"), grid(seq=600)],
}
# the intended differences, each as a row of its own (next to the pairs that the order above already gives)
EXTRA = {
    # drop_p is tested AFTER batch == 0 and after alignment here ...
    "uniir_attention_fwd_ex": [{"batch": 0, "drop_p": 1.5}, {"q": MIS, "drop_p": 1.5}, {"tq": 513, "q_ld": 132, "drop_p": 1.5}],
    "uniir_attention_fwd_rows": [{"batch": 0, "drop_p": 1.5}, {"q": MIS, "drop_p": 1.5}],
    # ... and of the backward's pointers only dq / dk / dv are tested for alignment: a misaligned input gets as far as drop_p
    "uniir_attention_bwd_ex": [{"batch": 0, "drop_p": 1.5}, {"dq": MIS, "drop_p": 1.5}] +
                              [{n: MIS, "drop_p": 1.5} for n in ("q", "k", "v", "out", "dout")],
    "uniir_attention_bwd_rows": [{"batch": 0, "drop_p": 1.5}, {"dk": MIS, "drop_p": 1.5}] +
                                [{n: MIS, "drop_p": 1.5} for n in ("q", "k", "v", "out", "dout")],
    # rel_fwd / rel_bwd test no alignment at all; their _long forms do
    "uniir_attention_rel_fwd": [{"batch": 0, "drop_p": 1.5}] + [{n: MIS, "drop_p": 1.5} for n in ("qkv", "out")],
    "uniir_attention_rel_bwd": [{"batch": 0, "drop_p": 1.5}] + [{n: MIS, "drop_p": 1.5} for n in ("qkv", "out", "dout", "dqkv")],
    # the _long forms test drop_p BEFORE batch == 0 (the pairs above have it; here with every later check failing as well)
    "uniir_attention_fwd_long": [{"batch": 0, "drop_p": 1.5, "tq": 0, "q_ld": 132, "q": MIS}, {"batch": 0, "tq": 0, "q_ld": 132}],
    "uniir_attention_bwd_long": [{"batch": 0, "drop_p": 1.5, "tq": 0, "dq_ld": 132, "dout": MIS}, {"batch": 0, "tk": 0, "dout": MIS}],
    "uniir_attention_rel_fwd_long": [{"batch": 0, "drop_p": 1.5, "seq": 0, "qkv": MIS}],
    "uniir_attention_rel_bwd_long": [{"batch": 0, "drop_p": 1.5, "seq": 0, "dqkv": MIS}, {"drel": None, "seq": 1025}],
    # a kv_ld that is no multiple of 8: UNIIR_EALIGN from the entry point, which tests it before the shared pooled form would (ESHAPE)
    "uniir_attention_one_fwd": [{"kv_ld": 260, "q": MIS}, {"kv_ld": 260, "tk": 1025}, {"batch": 0, "kv_ld": 260}],
    "uniir_attention_one_bwd": [{"kv_ld": 260, "tk": 1025}, {"batch": 0, "dkv_ld": 260}],
    # the dense / packed forms: the sequence limit depends on causal and row_off, not on the entry point
    "uniir_attention_fwd": [{"seq": 1024, "causal": 1}, {"batch": 0, "seq": 2000}],
    "uniir_attention_fwd_f16": [{"seq": 1024, "row_off": PTR, "qkv": MIS}],
}


def is_ptr(ctype):
    return ctype is C.c_void_p


def build_args(fn, change):
    """the argument list of one row in the JSON encoding: 'p:<offset>' / None for pointers, numbers (or 'nan') otherwise"""
    names, types = ARGS[fn], _lib.SIGNATURES[fn][1]
    assert len(names) == len(types), fn
    unknown = set(change) - set(names)
    assert not unknown, (fn, unknown)
    out = []
    for slot, (n, t) in enumerate(zip(names, types)):
        if is_ptr(t):
            dflt = None if (n in NULL_BY_DEFAULT or (n.endswith("row_off") and fn in OPTIONAL_ROW_OFF)) else PTR
            v = change.get(n, dflt)
            out.append(None if v is None else f"p:{256 * (slot + 1) + (2 if v == MIS else 0)}")
        else:
            out.append(change.get(n, GOOD.get(n)))
            assert out[-1] is not None, (fn, n)
    return out


def to_ctypes(fn, args, base):
    """JSON row -> the values of the call (the test decodes a row the same way)"""
    vals = []
    for a, t in zip(args, _lib.SIGNATURES[fn][1]):
        if is_ptr(t):
            vals.append(None if a is None else base + int(a[2:]))
        else:
            vals.append(math.nan if a == "nan" else a)
    return vals


def rows_of(fn):
    checks = CHECKS[fn]
    for i, variants in enumerate(checks):
        for v in variants:
            yield f"branch {i}", v
    for i in range(len(checks) - 1):
        a, b = checks[i][0], checks[i + 1][0]
        if set(a) & set(b):
            continue
        yield f"branches {i} and {i + 1} together", {**a, **b}
    for v in EXTRA.get(fn, []):
        yield "difference", v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=_lib.LIB_PATH)
    ap.add_argument("--commit", required=True, help="the commit the library was built from")
    opt = ap.parse_args()
    lib = C.CDLL(opt.lib)
    raw = C.create_string_buffer(BUF_BYTES + 256)
    base = (C.addressof(raw) + 255) & ~255
    pattern = bytes((7 * i + 3) & 255 for i in range(BUF_BYTES))
    cases = []
    for fn in ARGS:
        f = getattr(lib, fn)
        f.restype, f.argtypes = _lib.SIGNATURES[fn]
        bi = ARGS[fn].index("batch")
        for kind, change in rows_of(fn):
            args = build_args(fn, change)
            C.memmove(base, pattern, BUF_BYTES)
            code = int(f(*to_ctypes(fn, args, base)))
            if code == ELAUNCH or not (code != 0 or args[bi] == 0):
                raise SystemExit(f"{fn} {change}: code {code} -- this row reaches a launch; it must not be in the table")
            assert C.string_at(base, BUF_BYTES) == pattern, (fn, change)
            cases.append({"fn": fn, "kind": kind, "change": {k: v for k, v in change.items()}, "args": args, "code": code})
    out = {"recorded_at": opt.commit, "buffer_bytes": BUF_BYTES, "argnames": ARGS, "cases": cases}
    with open(os.path.join(HERE, "g17_attention_refusals.json"), "w") as fh:
        head = {k: v for k, v in out.items() if k != "cases"}          # one row per line: a diff of the table reads row by row
        fh.write(json.dumps(head, indent=1)[:-2] + ',\n "cases": [\n')
        fh.write(",\n".join("  " + json.dumps(c) for c in cases) + "\n ]\n}\n")
    by = {}
    for c in cases:
        by[c["code"]] = by.get(c["code"], 0) + 1
    print("g17 ok:", len(cases), "rows over", len(ARGS), "entry points; codes", dict(sorted(by.items())))


if __name__ == "__main__":
    main()
