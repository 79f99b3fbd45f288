"""What the 17 attention entry points answer to calls they refuse (CPU: a refused call returns before any HIP call).  The table is
tests/golden/g17_attention_refusals.json, recorded by tests/golden/make_golden_refusals.py from the library as it was BEFORE the
attention host layer was rebuilt on shared argument builders and check helpers ("recorded_at" in the file): per entry point one row
per refusal branch, one per pair of neighbouring branches failing together (which check wins), and the intended differences
between the entry points.  Every row must give the recorded code and leave the host buffer its pointers lie in untouched."""
import ctypes as C
import json
import math
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "g17_attention_refusals.json")) as _f:
    TABLE = json.load(_f)
FUNCS = sorted(TABLE["argnames"])
ELAUNCH = -4


def test_the_table_covers_the_17_attention_entry_points():
    from uniir_amd import _lib
    bound = {n for n in _lib.SIGNATURES if n.startswith("uniir_attention_") and n != "uniir_attention_f32_fwd"}
    assert len(FUNCS) == 17 and set(FUNCS) == bound
    assert {c["fn"] for c in TABLE["cases"]} == bound
    for fn in FUNCS:
        kinds = {c["kind"].split()[0] for c in TABLE["cases"] if c["fn"] == fn}
        assert {"branch", "branches"} <= kinds, (fn, kinds)
        assert len(TABLE["argnames"][fn]) == len(_lib.SIGNATURES[fn][1]), fn


@pytest.mark.parametrize("fn", FUNCS)
def test_refused_calls_return_the_recorded_code_and_write_nothing(fn):
    from uniir_amd import _lib
    lib = _lib.load()
    types = _lib.SIGNATURES[fn][1]
    bi = TABLE["argnames"][fn].index("batch")
    cases = [c for c in TABLE["cases"] if c["fn"] == fn]
    # no row may reach a launch: checked for ALL rows before the first call
    for c in cases:
        assert (c["code"] != 0 or c["args"][bi] == 0) and c["code"] != ELAUNCH, c
    n = TABLE["buffer_bytes"]
    raw = C.create_string_buffer(n + 256)
    base = (C.addressof(raw) + 255) & ~255
    pattern = bytes((7 * i + 3) & 255 for i in range(n))
    f = getattr(lib, fn)
    for c in cases:
        vals = []
        for a, t in zip(c["args"], types):
            if t is C.c_void_p:
                assert a is None or 0 < int(a[2:]) < n - 4096, c
                vals.append(None if a is None else base + int(a[2:]))
            else:
                vals.append(math.nan if a == "nan" else a)
        C.memmove(base, pattern, n)
        code = f(*vals)
        assert code == c["code"], (c["kind"], c["change"], code, c["code"])
        assert C.string_at(base, n) == pattern, (c["kind"], c["change"])
