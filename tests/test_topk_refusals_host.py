"""What the fp16 top-k entry points answer to calls they refuse (CPU: every check runs before any HIP call, so a refused call never
reaches a launch).  One table row per refusal branch: a valid call with ONE argument changed.  Every row must give the stated code
and leave the host buffer its pointers lie in untouched.  Also here, because it needs no device either: zero-sized requests of the
workspace functions, the sweep-width setting, and the restated workspace sizes of tests/topk_cases.py against the library's."""
import ctypes as C

import pytest

import topk_cases as T

OK, EINVAL, ESHAPE, EALIGN = 0, -1, -2, -3
N = 1 << 16                         # bytes of the host buffer the pointers lie in
ROWS, DIM, NQ, K, KC = 1000, 768, 4, 10, 18
BIG_ROWS = 1398102                  # BIG_ROWS * 768 * 2 >= 2^31 (1398101 rows stay below)
assert BIG_ROWS * 768 * 2 >= 2 ** 31 > (BIG_ROWS - 1) * 768 * 2
PTR = ("pool", "inv", "ids", "q", "qinv", "cand", "cscore", "exact", "out_s", "out_i", "ws", "scores")
OFF = {n: 256 * (i + 1) for i, n in enumerate(PTR)}           # distinct 256-byte aligned offsets

# entry point -> (argument names in ABI order, the stream excluded; the valid call)
VALID = {
    "uniir_topk_ip": (("pool", "inv", "ids", "rows", "dim", "q", "nq", "k", "out_s", "out_i", "ws", "ws_bytes"),
                      dict(rows=ROWS, dim=DIM, nq=NQ, k=K, ws_bytes="ip")),
    "uniir_topk_coarse": (("pool", "inv", "rows", "dim", "q", "nq", "kc", "cand", "cscore", "ws", "ws_bytes"),
                          dict(rows=ROWS, dim=DIM, nq=NQ, kc=KC, ws_bytes="coarse")),
    "uniir_topk_rescore": (("pool", "inv", "ids", "rows", "dim", "q", "qinv", "nq", "cand", "ncand", "k", "exact", "out_s", "out_i"),
                           dict(rows=ROWS, dim=DIM, nq=NQ, ncand=576, k=K)),
    "uniir_topk_merge": (("scores", "ids", "nshard", "nq", "k", "out_s", "out_i"), dict(nshard=3, nq=NQ, k=K)),
    "uniir_topk_merge_ex": (("scores", "ids", "nshard", "nq", "k_in", "k_out", "out_s", "out_i"), dict(nshard=3, nq=NQ, k_in=K, k_out=25)),
}
# (entry point, argument, value | "null" | ("misaligned", bytes) | "short", code)
ROWS_OF_TABLE = []


def _rows(fn, code, arg_values):
    for a, v in arg_values:
        ROWS_OF_TABLE.append((fn, a, v, code))


_rows("uniir_topk_ip", EINVAL, [(p, "null") for p in ("pool", "inv", "q", "out_s", "out_i", "ws")]
      + [("rows", 0), ("rows", -1), ("nq", 0), ("nq", -3), ("k", 0), ("k", -1), ("ws_bytes", "short")])
_rows("uniir_topk_ip", ESHAPE, [("k", 57), ("k", 64), ("dim", 96), ("dim", 32), ("dim", 0), ("dim", -64), ("rows", BIG_ROWS), ("rows", 1 << 31)])
_rows("uniir_topk_ip", EALIGN, [("pool", ("misaligned", 8)), ("q", ("misaligned", 8)), ("inv", ("misaligned", 4)), ("ws", ("misaligned", 128)),
                                ("ws", ("misaligned", 16))])
_rows("uniir_topk_coarse", EINVAL, [(p, "null") for p in ("pool", "inv", "q", "cand", "ws")]
      + [("rows", 0), ("rows", -1), ("nq", 0), ("nq", -3), ("kc", 0), ("ws_bytes", "short")])
_rows("uniir_topk_coarse", ESHAPE, [("kc", 65), ("dim", 48), ("dim", 8), ("dim", 0), ("rows", BIG_ROWS), ("rows", 1 << 31)])
_rows("uniir_topk_coarse", EALIGN, [("pool", ("misaligned", 8)), ("q", ("misaligned", 8)), ("inv", ("misaligned", 4)), ("ws", ("misaligned", 8))])
_rows("uniir_topk_rescore", EINVAL, [(p, "null") for p in ("pool", "inv", "q", "qinv", "cand", "exact", "out_s", "out_i")]
      + [("rows", 0), ("nq", 0), ("nq", -1), ("ncand", 0), ("k", 0), ("k", -1)])
_rows("uniir_topk_rescore", ESHAPE, [("dim", 100), ("dim", 4), ("dim", 0), ("dim", -8)])
_rows("uniir_topk_rescore", EALIGN, [("pool", ("misaligned", 8)), ("q", ("misaligned", 8))])
for _fn, _ks in (("uniir_topk_merge", ("k",)), ("uniir_topk_merge_ex", ("k_in", "k_out"))):
    _rows(_fn, EINVAL, [(p, "null") for p in ("scores", "ids", "out_s", "out_i")] + [("nshard", 0), ("nshard", -1), ("nq", 0), ("nq", -2)]
          + [(k_, v) for k_ in _ks for v in (0, -1)])


def _need(lib, which, args):
    if which == "ip":
        return lib.uniir_topk_ip_workspace_bytes_ex(args["nq"], args["k"], args["rows"], args["dim"])
    return lib.uniir_topk_workspace_bytes(args["nq"], args["kc"], args["rows"])


def test_the_table_covers_every_entry_point_and_code():
    from uniir_amd import _lib
    for fn, (names, _) in VALID.items():
        assert len(names) + 1 == len(_lib.SIGNATURES[fn][1]), fn          # + the stream
        codes = {r[3] for r in ROWS_OF_TABLE if r[0] == fn}
        assert EINVAL in codes and (fn.startswith("uniir_topk_merge") or {ESHAPE, EALIGN} <= codes), (fn, codes)


@pytest.mark.parametrize("fn", sorted(VALID))
def test_refused_calls_return_the_stated_code_and_write_nothing(fn):
    from uniir_amd import _lib
    lib = _lib.load()
    raw = C.create_string_buffer(N + 256)
    base = (C.addressof(raw) + 255) & ~255
    pattern = bytes((7 * i + 3) & 255 for i in range(N))
    names, valid = VALID[fn]
    f = getattr(lib, fn)
    for _, arg, val, code in (r for r in ROWS_OF_TABLE if r[0] == fn):
        assert code in (EINVAL, ESHAPE, EALIGN)
        args = {n: base + OFF[n] for n in names if n in OFF}
        args.update(valid)
        if val == "short":
            args[arg] = _need(lib, valid[arg], args) - 1
        elif val == "null":
            args[arg] = None
        elif isinstance(val, tuple):
            args[arg] = base + OFF[arg] + val[1]
        else:
            args[arg] = val
        if isinstance(args.get("ws_bytes"), str):                # after the change: the requirement of the call as made
            args["ws_bytes"] = _need(lib, valid["ws_bytes"], args)
        C.memmove(base, pattern, N)
        got = f(*[args[n] for n in names], None)
        assert got == code, (fn, arg, val, got, code)
        assert C.string_at(base, N) == pattern, (fn, arg, val)


def test_zero_sized_requests_need_no_workspace():
    from uniir_amd import _lib
    lib = _lib.load()
    assert lib.uniir_topk_ip_workspace_bytes_ex(NQ, K, ROWS, DIM) > 0
    for nq, k, rows, dim in ((0, K, ROWS, DIM), (NQ, 0, ROWS, DIM), (NQ, K, 0, DIM), (NQ, K, ROWS, 0), (-1, K, ROWS, DIM), (NQ, K, -5, DIM)):
        assert lib.uniir_topk_ip_workspace_bytes_ex(nq, k, rows, dim) == 0
        assert dim == 0 or lib.uniir_topk_ip_workspace_bytes(nq, k, rows) == 0
        assert dim == 0 or lib.uniir_topk_workspace_bytes(nq, k, rows) == 0


def test_the_sweep_width_setting_refuses_what_it_cannot_take():
    from uniir_amd import _lib
    lib = _lib.load()
    try:
        for bad in (-1, 1025, 1 << 20):
            assert lib.uniir_topk_set_chunk(bad) == EINVAL
            assert lib.uniir_topk_ip_sweep_queries(768, 40000) == 256          # a refused value changes nothing
        for good in (64, 1, 1024):
            assert lib.uniir_topk_set_chunk(good) == OK
            assert lib.uniir_topk_ip_sweep_queries(768, 40000) == good == T.sweep_queries(768, 40000, good)
    finally:
        assert lib.uniir_topk_set_chunk(0) == OK
    assert lib.uniir_topk_ip_sweep_queries(768, 32768) == 256 and lib.uniir_topk_ip_sweep_queries(768, 32752) == 1024
    assert lib.uniir_topk_ip_sweep_queries(512, 40000) == 1024


def test_the_restated_sizes_equal_the_librarys():
    from uniir_amd import _lib
    lib = _lib.load()
    try:
        for c in T.CASES:
            if c.kind == "ip":
                assert lib.uniir_topk_set_chunk(c.chunk) == OK
                assert lib.uniir_topk_ip_workspace_bytes_ex(c.nq, c.k, c.rows, c.dim) == T.ip_workspace_bytes(c.nq, c.k, c.rows, c.dim, c.chunk), c.name
                assert lib.uniir_topk_ip_sweep_queries(c.dim, c.rows) == T.sweep_queries(c.dim, c.rows, c.chunk), c.name
            elif c.kind == "coarse":
                assert lib.uniir_topk_workspace_bytes(c.nq, c.k + 8, c.rows) == T.workspace_bytes(c.nq, c.k + 8, c.rows), c.name
                assert lib.uniir_topk_ncand(c.nq, c.k + 8) == T.ncand(c.nq, c.k + 8), c.name
    finally:
        assert lib.uniir_topk_set_chunk(0) == OK
