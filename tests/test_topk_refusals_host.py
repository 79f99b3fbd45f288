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

# entry point[:variant of the valid call] -> (argument names in ABI order, the stream excluded; the valid call)
VALID = {
    "uniir_topk_ip": (("pool", "inv", "ids", "rows", "dim", "q", "nq", "k", "out_s", "out_i", "ws", "ws_bytes"),
                      dict(rows=ROWS, dim=DIM, nq=NQ, k=K, ws_bytes="ip")),
    "uniir_topk_ip_multi": (("pool", "inv", "ids", "rows", "dim", "q", "nq", "k", "out_s", "out_i", "ws", "ws_bytes"),
                            dict(rows=ROWS, dim=DIM, nq=NQ, k=K, ws_bytes="multi")),          # below 2 GiB: uniir_topk_ip's checks
    "uniir_topk_ip_multi:big": (("pool", "inv", "ids", "rows", "dim", "q", "nq", "k", "out_s", "out_i", "ws", "ws_bytes"),
                                dict(rows=BIG_ROWS, dim=DIM, nq=NQ, k=K, ws_bytes="multi")),  # two sub-shards (a refused call touches no row)
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
for _fn, _more in (("uniir_topk_ip_multi", ()), ("uniir_topk_ip_multi:big", ("ids",))):
    _rows(_fn, EINVAL, [(p, "null") for p in ("pool", "inv", "q", "out_s", "out_i", "ws") + _more]
          + [("rows", 0), ("rows", -1), ("nq", 0), ("nq", -3), ("k", 0), ("k", -1), ("ws_bytes", "short")])
    _rows(_fn, ESHAPE, [("k", 57), ("dim", 96), ("rows", 1 << 31)])
    _rows(_fn, EALIGN, [("pool", ("misaligned", 8)), ("q", ("misaligned", 8)), ("inv", ("misaligned", 4)), ("ws", ("misaligned", 128))])
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
    if which == "multi":
        return lib.uniir_topk_ip_multi_workspace_bytes(args["nq"], args["k"], args["rows"], args["dim"])
    if which == "ip":
        return lib.uniir_topk_ip_workspace_bytes_ex(args["nq"], args["k"], args["rows"], args["dim"])
    return lib.uniir_topk_workspace_bytes(args["nq"], args["kc"], args["rows"])


def test_the_table_covers_every_entry_point_and_code():
    from uniir_amd import _lib
    for fn, (names, _) in VALID.items():
        assert len(names) + 1 == len(_lib.SIGNATURES[fn.split(":")[0]][1]), fn          # + the stream
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
    f = getattr(lib, fn.split(":")[0])
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


MULTI_DIMS = (512, 768, 1024)
MULTI_ROWS = (1_398_101, 1_398_102, 1_500_016, 1_500_032, 2_200_000, 5_600_000)
MULTI_NQ = (1, 64, 65, 256, 257, 300, 1024, 1100)
MULTI_K = (1, 10, 56)
MULTI_CHUNKS = (0, 64)


def test_the_restated_multi_sizes_equal_the_librarys():
    """sub-shard rows, sub-shard count and uniir_topk_ip_multi_workspace_bytes over shards on both sides of the 2-GiB bound, and
    retrieval.subshard_bounds against the library's rule.  (Passed as written against the library before the host layer was
    consolidated: the sizes are the behaviour pin of that refactor.)"""
    from uniir_amd import _lib, retrieval
    lib = _lib.load()
    try:
        for chunk in MULTI_CHUNKS:
            assert lib.uniir_topk_set_chunk(chunk) == OK
            for dim in MULTI_DIMS:
                for rows in MULTI_ROWS:
                    per, nsub, last = T.subshards(rows, dim)
                    assert lib.uniir_topk_subshard_rows(rows, dim) == per and 0 < last <= per and (nsub - 1) * per + last == rows
                    assert (nsub > 1) == (rows * dim * 2 >= 2 ** 31)
                    bounds = retrieval.subshard_bounds(rows, dim)
                    assert bounds == [(z * per, min((z + 1) * per, rows)) for z in range(nsub)], (rows, dim)
                    for nq in MULTI_NQ:
                        for k in MULTI_K:
                            assert lib.uniir_topk_ip_multi_workspace_bytes(nq, k, rows, dim) == T.multi_workspace_bytes(nq, k, rows, dim, chunk), \
                                (rows, dim, nq, k, chunk)
    finally:
        assert lib.uniir_topk_set_chunk(0) == OK
    for nq, k, rows, dim in ((0, K, BIG_ROWS, DIM), (NQ, 0, BIG_ROWS, DIM), (NQ, K, 0, DIM), (NQ, K, BIG_ROWS, 0)):
        assert lib.uniir_topk_ip_multi_workspace_bytes(nq, k, rows, dim) == 0 == T.multi_workspace_bytes(nq, k, rows, dim)
    assert lib.uniir_topk_subshard_rows(0, DIM) == 0 == lib.uniir_topk_subshard_rows(ROWS, 0)


# ------------------------------------------------------------------------------------------------ the library's plan
SCAN_NAME = ("topk_stream_kernel<{nk}>", "topk_stream2_kernel<{nk},2>", "topk_stream5_kernel<2,2>", "topk_stream5_kernel<4,2>",
             "topk_gmax_pp_kernel<true,2>", "topk_gmax_pp_kernel<false,2>", "topk_gmax_pp_kernel<false,0>", "topk_gmax_kernel<2>")
SEL_NAME = ("topk_gsel_kernel<1024,true>", "topk_gsel_kernel<1024,false>", "topk_gsel_kernel<256>")
TAIL_NAME = {4: "topk_tail_select_rescore_kernel<4,3,4>", 2: "topk_tail_select_rescore_kernel<2,5,2>", 1: "topk_tail_select_rescore_kernel<1,5,2>"}
NCUS = (256, 64, 304, 320)          # the MI355X; a quarter of it; two counts whose 4 ncu waves exceed the 1024 the wave maxima hold


def _planned_sweep(dim, k, ncand, scan, waves, tail, select, ncu):
    """the names topk_cases gives the launches of one planned sweep"""
    assert waves in (0, 4 * ncu)
    names = (SCAN_NAME[scan].format(nk=dim // 32),)
    if tail == 1:
        return names + (TAIL_NAME[select], "gsel_hier" if waves else "gsel_body<1024,true>", "topk_tail_sort_kernel")
    return names + (SEL_NAME[select],) + T.rescore_path(dim, ncand)


def _planned_sweeps(p, dim, k, ncu):
    """-> [(queries, names)] of the full-width sweep and the remainder sweep of a plan"""
    out = [(p.sweep_queries, _planned_sweep(dim, k, p.ncand, p.scan, p.waves, p.tail, p.select, ncu))]
    if p.rem_queries:
        out.append((p.rem_queries, _planned_sweep(dim, k, p.ncand, p.rem_scan, p.rem_waves, p.rem_tail, p.rem_select, ncu)))
    return out


@pytest.mark.parametrize("ncu", NCUS)
def test_the_plan_equals_the_restated_dispatch_for_every_search_case(ncu):
    """uniir_topk_plan against topk_cases.sweep_path / scan_path / fused_tail_ok / wave_maxima: every "ip" case (the kinds that
    call the op-level entry points have no search plan), sweep by sweep, on four device sizes"""
    from uniir_amd import _lib
    lib = _lib.load()
    try:
        for c in (c for c in T.CASES if c.kind == "ip"):
            assert lib.uniir_topk_set_chunk(c.chunk) == OK
            p = _lib.topk_plan(c.rows, c.dim, c.nq, c.k, ncu)
            width = min(c.nq, T.sweep_queries(c.dim, c.rows, c.chunk))
            assert (p.sweep_queries, p.rem_queries, p.nsub, p.batched) == (width, c.nq % width, 1, 0), c.name
            assert (p.subshard_rows, p.last_rows, p.ncand) == (c.rows, c.rows, T.ncand(width, c.k + 8)), c.name
            assert p.workspace_bytes == T.ip_workspace_bytes(c.nq, c.k, c.rows, c.dim, c.chunk), c.name
            seen = []
            for n, names in _planned_sweeps(p, c.dim, c.k, ncu):
                assert names == T.sweep_path(c.rows, c.dim, n, c.k, ncu), (c.name, n)
                scan, sel, wm = T.scan_path(c.rows, c.dim, n, ncu)
                waves = p.waves if n == width else p.rem_waves
                assert waves == (4 * ncu if wm else 0), (c.name, n)            # (also where an unfused tail leaves them unread)
                assert (p.tail if n == width else p.rem_tail) == int(sel >= 1 and T.fused_tail_ok(c.rows, c.dim, c.k + 8)), (c.name, n)
                seen += [x for x in names if x not in seen]
            assert tuple(seen) == T.path(c.rows, c.dim, c.nq, c.k, ncu, c.chunk), c.name
    finally:
        assert lib.uniir_topk_set_chunk(0) == OK
    assert any(T.wave_maxima(T.cdiv(c.rows, T.TK_G), 64) != T.wave_maxima(T.cdiv(c.rows, T.TK_G), 304) for c in T.CASES if c.kind == "ip")


def test_the_plan_equals_the_restated_batched_rule():
    """the multi search over the grid of the size test: sub-shards, sizes, the batched decision and, where batched, the launches of
    both sweeps; then the statements test_topk_ip_multi_equals_the_merge_of_sub_shard_searches makes about its shapes, on shapes
    no small device case can reach"""
    from uniir_amd import _lib
    lib = _lib.load()
    batched = {}
    try:
        for chunk in MULTI_CHUNKS:
            assert lib.uniir_topk_set_chunk(chunk) == OK
            for dim in MULTI_DIMS:
                for rows in MULTI_ROWS:
                    per, nsub, last = T.subshards(rows, dim)
                    for nq in MULTI_NQ:
                        for k in MULTI_K:
                            for ncu in (256, 64):
                                p = _lib.topk_plan(rows, dim, nq, k, ncu)
                                what = (rows, dim, nq, k, chunk, ncu)
                                assert (p.nsub, p.subshard_rows, p.last_rows) == (nsub, per, last), what
                                assert p.workspace_bytes == T.multi_workspace_bytes(nq, k, rows, dim, chunk), what
                                assert p.batched == int(T.multi_batched(rows, dim, nq, k, chunk)), what
                                assert p.sweep_queries == min(nq, T.sweep_queries(dim, per, chunk)), what
                                batched[what] = p.batched
                                for n, names in _planned_sweeps(p, dim, k, ncu):
                                    want = T.multi_sweep_path(rows, dim, n, k, ncu)[:4] if p.batched else T.sweep_path(per, dim, n, k, ncu)
                                    assert names == want, (what, n)
    finally:
        assert lib.uniir_topk_set_chunk(0) == OK
    for ncu in (256, 64):
        assert all(batched[5_600_000, 768, nq, 10, 0, ncu] for nq in (64, 256, 1024))
        assert not any(batched[1_500_016, 768, nq, 10, 0, ncu] for nq in MULTI_NQ)            # an odd number of groups in the last sub-shard
        assert batched[2_200_000, 512, 64, 10, 0, ncu] and not batched[2_200_000, 512, 300, 10, 0, ncu]
        assert batched[2_200_000, 512, 300, 10, 64, ncu]                                      # ... but in 64-query sweeps it is
        assert batched[1_500_032, 768, 300, 10, 0, ncu]
    p = _lib.topk_plan(1_500_032, 768, 300, 10, 256)                                          # batched in both sweeps: 256 + 44
    assert (p.sweep_queries, p.rem_queries, p.scan, p.rem_scan) == (256, 44, 3, 1) and p.tail == p.rem_tail == 1
    # the hierarchical selection needs the wave maxima of EVERY sub-shard: 700 000-row sub-shards leave them on 256 compute units
    # (43 groups per wave) and not on 64 (171)
    assert _lib.topk_plan(5_600_000, 768, 64, 10, 256).waves == 1024 and _lib.topk_plan(5_600_000, 768, 64, 10, 64).waves == 0
    assert _lib.topk_plan(5_600_000, 768, 64, 10, 256).select == 1 and _lib.topk_plan(1_500_032, 768, 64, 10, 256).select == 2


def test_the_plan_query_refuses_what_the_searches_refuse():
    from uniir_amd import _lib
    lib = _lib.load()
    out = _lib.TopkPlan()
    for args, code in (((0, DIM, NQ, K, 256), EINVAL), ((ROWS, 0, NQ, K, 256), EINVAL), ((ROWS, DIM, 0, K, 256), EINVAL),
                       ((ROWS, DIM, NQ, 0, 256), EINVAL), ((ROWS, DIM, NQ, K, 0), EINVAL), ((ROWS, DIM, NQ, 57, 256), ESHAPE),
                       ((ROWS, 96, NQ, K, 256), ESHAPE), ((1 << 31, DIM, NQ, K, 256), ESHAPE)):
        assert lib.uniir_topk_plan(*args, C.byref(out)) == code, args
    assert lib.uniir_topk_plan(ROWS, DIM, NQ, K, 256, None) == EINVAL
