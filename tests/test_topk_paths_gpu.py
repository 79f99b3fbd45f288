"""The fp16 top-k search of the C ABI on every dispatch path against the exact oracle (tests/topk_cases.py holds the case table, the
restated dispatch, the generators and the references): uniir_topk_ip, uniir_topk_coarse + uniir_topk_rescore, uniir_topk_rescore on
hand-made shortlists, uniir_topk_merge / uniir_topk_merge_ex.  Scores must equal the reference bit for bit and ids exactly; the
queries flagged `mass_ties` must get a VALID answer instead (topk_cases.check_valid_answer, include/uniir_hip.h [TOPK]).

Calls go through the ctypes handle on the test's own buffers:
  * out_scores / out_ids lie inside larger buffers filled with a NaN bit pattern / a sentinel id: GUARD_LISTS lists in front and
    behind must come back bit for bit;
  * pool, queries, inverse norms and ids are followed by guard rows.  The pool's hold twice the first query in fp16 -- they would
    win every search if a ragged group or tile read them as live rows -- and their inverse norms are 1.0 so that such a read is not
    masked; the queries' hold NaN; every input must come back bit for bit as well;
  * the workspace is exactly uniir_topk_ip_workspace_bytes_ex (uniir_topk_workspace_bytes for the op-level calls) bytes, 256-byte
    aligned, inside a guarded buffer;
  * every case runs twice, on a workspace (and every scratch array) filled with 0xFF and with 0x00 bytes: both results must be
    torch.equal and equal the reference -- a result that depends on stale scratch differs in one of them.
Inverse norms come from uniir_pool_inv_norms (pinned by test_glue_paths_gpu.py).  Every case prints an OBS line with the path()
of the device's real compute-unit count (profiles/topk_paths.txt keeps a run's lines); on a device where that differs from the
path the case names, the case is skipped with that reason instead of passing on another kernel.  The second of the two runs is
recorded by torch.profiler: the search kernels it launched must be exactly those of that path (KERNELS line), so a case cannot pass
on a kernel it does not name."""
import ctypes as C
import faulthandler
import re

import numpy as np
import pytest
import torch

import topk_cases as T

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD_ROWS = 256            # rows behind the pool / inverse norms / ids: a whole 256-row tile
GUARD_QUERIES = 64
GUARD_LISTS = 8             # [k] lists in front of and behind the outputs
GUARD_BYTES = 4096          # around the workspace and behind scratch arrays
NAN32, NAN16, SENTINEL_ID, GUARD_BYTE = 0x7FC00011, 0x7E01, -0x5A5A5A5A5A5A5A5B, 0xA5
ERR = {"EINVAL": -1, "ESHAPE": -2, "EALIGN": -3}
CASE_SECONDS = 120          # a case takes a few seconds; a hung kernel ends the run here instead of at the runner's limit


def _lib():
    from uniir_amd import _lib
    return _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t, byte_off=0):
    return C.c_void_p(t.data_ptr() + byte_off)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _dev(a):
    """a numpy array (possibly read-only) on the device"""
    return torch.from_numpy(np.array(a)).to(DEV)


class Inputs:
    """device copies of pool / ids / queries with their guard rows, the inverse norms from uniir_pool_inv_norms, and clones to
    compare with after the calls"""

    def __init__(self, pool, ids, queries):
        self.rows, self.dim = pool.shape
        self.nq = queries.shape[0]
        q16 = _dev(queries.view(np.int16))
        guard = (q16[0].view(torch.float16).float() * 2).half().view(torch.int16)
        self.pool = torch.cat([_dev(pool.view(np.int16)), guard.expand(GUARD_ROWS, -1)]).contiguous()
        self.queries = torch.cat([q16, torch.full((GUARD_QUERIES, self.dim), NAN16, dtype=torch.int16, device=DEV)]).contiguous()
        self.ids = None
        if ids is not None:
            self.ids = torch.cat([_dev(ids), torch.full((GUARD_ROWS,), SENTINEL_ID, dtype=torch.int64, device=DEV)])
        self.inv = torch.ones(self.rows + GUARD_ROWS, device=DEV)
        self.qinv = torch.ones(self.nq + GUARD_QUERIES, device=DEV)
        assert _lib().uniir_pool_inv_norms(_p(self.pool), self.rows, self.dim, _p(self.inv), _stream()) == 0
        assert _lib().uniir_pool_inv_norms(_p(self.queries), self.nq, self.dim, _p(self.qinv), _stream()) == 0
        torch.cuda.synchronize()
        assert bool((self.inv[self.rows:] == 1).all()) and bool((self.qinv[self.nq:] == 1).all())
        self._keep = [t.clone() for t in self._all()]

    def _all(self):
        return [t for t in (self.pool, self.queries, self.ids, self.inv, self.qinv) if t is not None]

    def assert_untouched(self):
        for t, k in zip(self._all(), self._keep):
            assert torch.equal(t, k), "an input or its guard rows changed"


class Outputs:
    """[nq][k] scores and ids inside guarded buffers"""

    def __init__(self, nq, k):
        self.nq, self.k = nq, k
        n = (nq + 2 * GUARD_LISTS) * k
        self.s = torch.full((n,), NAN32, dtype=torch.int32, device=DEV)
        self.i = torch.full((n,), SENTINEL_ID, dtype=torch.int64, device=DEV)

    def ptrs(self):
        return _p(self.s, GUARD_LISTS * self.k * 4), _p(self.i, GUARD_LISTS * self.k * 8)

    def take(self):
        """-> (scores, ids) on the device; the guard lists must be intact"""
        torch.cuda.synchronize()
        g, n = GUARD_LISTS * self.k, self.nq * self.k
        for t, fill in ((self.s, NAN32), (self.i, SENTINEL_ID)):
            assert bool((t[:g] == fill).all()), "a write in front of the output"
            assert bool((t[g + n:] == fill).all()), "a write behind the output"
        return self.s[g:g + n].view(torch.float32).view(self.nq, self.k).clone(), self.i[g:g + n].view(self.nq, self.k).clone()


class Scratch:
    """`nbytes` bytes at a 256-byte aligned address, pre-filled with `fill`, inside a guarded buffer"""

    def __init__(self, nbytes, fill):
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + 2 * GUARD_BYTES + 256,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.off = GUARD_BYTES + (-(self.buf.data_ptr() + GUARD_BYTES)) % 256
        self.buf[self.off:self.off + self.nbytes] = fill
        assert (self.buf.data_ptr() + self.off) % 256 == 0

    def ptr(self):
        return _p(self.buf, self.off)

    def assert_guards(self):
        torch.cuda.synchronize()
        assert bool((self.buf[:self.off] == GUARD_BYTE).all()), "a write in front of the workspace"
        assert bool((self.buf[self.off + self.nbytes:] == GUARD_BYTE).all()), "a write behind the workspace"


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else a.dtype),
                                                                        b.view(np.uint32 if b.dtype == np.float32 else b.dtype))


def _observe(c):
    """the OBS line; skips on a device where the host layer takes another path than the case names"""
    here, named = T.case_path(c, _ncu()), T.case_path(c, T.NCU)
    data = [r for r in c.reach if r in T.DATA_BRANCHES]
    print(f"\nOBS {c.name} ncu={_ncu()} [{' + '.join(here)}]" + (f" data: {' + '.join(data)}" if data else "")
          + (f" mass_ties: queries {list(c.mass_ties)}" if c.mass_ties else ""))
    if here != named:
        pytest.skip(f"{_ncu()} compute units: the host layer takes {here}, the case names {named}")


KERNEL = re.compile(r"^(topk_|rescore_|final_sort_kernel|merge_rank_kernel|merge_shards_kernel)")
SEEN = {}                   # case -> the search kernels the profiler saw it launch


def _expected_kernels(path):
    """the kernel names of a path as the profiler spells them (spaces removed): the selection templates inside the fused tail and the
    branch of final_sort_kernel are no kernels of their own"""
    names = {n.split("[")[0] for n in path if not n.startswith(("gsel_hier", "gsel_body"))}
    return {"topk_gsel_kernel<256,false>" if n == "topk_gsel_kernel<256>" else n for n in names}


def _profiled(c, run):
    """run() under torch.profiler; the search kernels it launches must be those of the case's path on this device"""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = run()
        torch.cuda.synchronize()
    names = {e.name.replace("void ", "").split("(")[0].replace(" ", "") for e in prof.events()
             if e.device_type == torch.autograd.DeviceType.CUDA}
    names = {n for n in names if KERNEL.match(n)}
    SEEN.setdefault(c.name, set()).update(names)
    print(f"KERNELS {c.name} {'  '.join(sorted(names)) if names else '(the profiler saw none)'}")
    if names:
        assert names == _expected_kernels(T.case_path(c, _ncu())), (c.name, sorted(names), T.case_path(c, _ncu()))
    return res


def _twice(c, run):
    """run(fill) for both fills -> the (scores, ids) of the first, as numpy; both must be torch.equal"""
    a, b = run(0xFF), _profiled(c, lambda: run(0x00))
    assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), "the result depends on stale scratch"
    return a[0].cpu().numpy(), a[1].cpu().numpy()


def _assert_equals_reference(c, d, got_s, got_i, want_s, want_i):
    k = c.k
    for q in range(got_s.shape[0]):
        if q in c.mass_ties:
            why = T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], k, got_s[q], got_i[q], want_s[q])
            assert why is None, (c.name, q, why, got_s[q], got_i[q], want_s[q], want_i[q])
    keep = np.array([q not in c.mass_ties for q in range(got_s.shape[0])])
    bad = np.argwhere((got_s.view(np.uint32) != want_s.view(np.uint32)) & keep[:, None])
    assert bad.size == 0, (c.name, "scores", bad[:5], got_s[bad[0][0]], want_s[bad[0][0]])
    bad = np.argwhere((got_i != want_i) & keep[:, None])
    assert bad.size == 0, (c.name, "ids", bad[:5], got_i[bad[0][0]], want_i[bad[0][0]])


def _search_ip(c, inp, fill):
    lib = _lib()
    need = lib.uniir_topk_ip_workspace_bytes_ex(c.nq, c.k, c.rows, c.dim)
    assert need == T.ip_workspace_bytes(c.nq, c.k, c.rows, c.dim, c.chunk), "the restated workspace size"
    ws, out = Scratch(need, fill), Outputs(c.nq, c.k)
    rc = lib.uniir_topk_ip(_p(inp.pool), _p(inp.inv), _p(inp.ids), c.rows, c.dim, _p(inp.queries), c.nq, c.k, *out.ptrs(),
                           ws.ptr(), need, _stream())
    assert rc == 0, rc
    res = out.take()
    ws.assert_guards()
    return res


IP = [c.name for c in T.CASES if c.kind == "ip"]


@pytest.mark.parametrize("name", IP)
def test_topk_ip_path(name):
    c = T.BY_NAME[name]
    _observe(c)
    d = T.build_ip(name)
    ref = T.reference_ip(name)
    want_s, want_i = np.ascontiguousarray(ref[0][:, :c.k]), np.ascontiguousarray(ref[1][:, :c.k])
    inp = Inputs(d["pool"], d["ids"], d["queries"])
    lib = _lib()
    assert lib.uniir_topk_set_chunk(c.chunk) == 0
    try:
        assert lib.uniir_topk_ip_sweep_queries(c.dim, c.rows) == T.sweep_queries(c.dim, c.rows, c.chunk)
        got_s, got_i = _twice(c, lambda fill: _search_ip(c, inp, fill))
    finally:
        assert lib.uniir_topk_set_chunk(0) == 0
    inp.assert_untouched()
    _assert_equals_reference(c, d, got_s, got_i, want_s, want_i)
    if c.rows < c.k:          # FAISS padding
        assert bool(np.isneginf(got_s[:, c.rows:]).all()) and bool((got_i[:, c.rows:] == -1).all())


def test_topk_ip_refuses_k_57_and_writes_nothing():
    c = T.BY_NAME["k56-fused"]
    d = T.build_ip(c.name)
    inp = Inputs(d["pool"], d["ids"], d["queries"])
    lib = _lib()
    need = lib.uniir_topk_ip_workspace_bytes_ex(c.nq, 57, c.rows, c.dim)
    ws, out = Scratch(need, 0xFF), Outputs(c.nq, 57)
    rc = lib.uniir_topk_ip(_p(inp.pool), _p(inp.inv), _p(inp.ids), c.rows, c.dim, _p(inp.queries), c.nq, 57, *out.ptrs(), ws.ptr(),
                           need, _stream())
    assert rc == ERR["ESHAPE"]
    torch.cuda.synchronize()
    assert bool((out.s == NAN32).all()) and bool((out.i == SENTINEL_ID).all())
    assert bool((ws.buf[ws.off:ws.off + need] == 0xFF).all())


# ------------------------------------------------------------------------------------------------ the op-level entry points
def _coarse_then_rescore(c, inp, fill):
    lib = _lib()
    kc = c.k + 8
    ncand = lib.uniir_topk_ncand(c.nq, kc)
    assert ncand == T.ncand(c.nq, kc)
    need = lib.uniir_topk_workspace_bytes(c.nq, kc, c.rows)
    assert need == T.workspace_bytes(c.nq, kc, c.rows), "the restated workspace size"
    ws = Scratch(need, fill)
    cand, cscore, exact = (Scratch(c.nq * n * 4, fill) for n in (ncand, kc, ncand))
    out = Outputs(c.nq, c.k)
    rc = lib.uniir_topk_coarse(_p(inp.pool), _p(inp.inv), c.rows, c.dim, _p(inp.queries), c.nq, kc, cand.ptr(), cscore.ptr(), ws.ptr(),
                               need, _stream())
    assert rc == 0, rc
    rc = lib.uniir_topk_rescore(_p(inp.pool), _p(inp.inv), _p(inp.ids), c.rows, c.dim, _p(inp.queries), _p(inp.qinv), c.nq, cand.ptr(),
                                ncand, c.k, exact.ptr(), *out.ptrs(), _stream())
    assert rc == 0, rc
    res = out.take()
    for s in (ws, cand, cscore, exact):
        s.assert_guards()
    idx = cand.buf[cand.off:cand.off + cand.nbytes].view(torch.int32)
    assert bool(((idx >= -1) & (idx < c.rows)).all()), "a shortlist entry that is no row of the pool"
    return res


@pytest.mark.parametrize("name", [c.name for c in T.CASES if c.kind == "coarse"])
def test_topk_coarse_then_rescore(name):
    c = T.BY_NAME[name]
    _observe(c)
    d = T.build_ip(name)
    ref = T.reference_ip(name)
    inp = Inputs(d["pool"], d["ids"], d["queries"])
    got_s, got_i = _twice(c, lambda fill: _coarse_then_rescore(c, inp, fill))
    inp.assert_untouched()
    _assert_equals_reference(c, d, got_s, got_i, np.ascontiguousarray(ref[0][:, :c.k]), np.ascontiguousarray(ref[1][:, :c.k]))


@pytest.mark.parametrize("name", [c.name for c in T.CASES if c.kind == "rescore"])
def test_topk_rescore_of_a_hand_made_shortlist(name):
    c = T.BY_NAME[name]
    _observe(c)
    d = T.build_shortlists(name)
    want_s, want_i = T.reference_shortlist(d, c.k)
    assert bool(np.isneginf(want_s[3, 4:]).all()) and bool((want_i[3, 4:] == -1).all())          # the generator: query 3 pads
    inp = Inputs(d["pool"], d["ids"], d["queries"])
    cand = torch.cat([_dev(d["cand"]).reshape(-1), torch.full((4096,), -1, dtype=torch.int32, device=DEV)])
    cand_keep = cand.clone()
    lib = _lib()

    def run(fill):
        exact, out = Scratch(c.nq * c.rows * 4, fill), Outputs(c.nq, c.k)
        rc = lib.uniir_topk_rescore(_p(inp.pool), _p(inp.inv), None if inp.ids is None else _p(inp.ids), T.SHORTLIST_POOL, c.dim,
                                    _p(inp.queries), _p(inp.qinv), c.nq, _p(cand), c.rows, c.k, exact.ptr(), *out.ptrs(), _stream())
        assert rc == 0, rc
        res = out.take()
        exact.assert_guards()
        return res

    got_s, got_i = _twice(c, run)
    inp.assert_untouched()
    assert torch.equal(cand, cand_keep)
    assert _same_bits(got_s, want_s), (got_s, want_s)
    assert np.array_equal(got_i, want_i), (got_i, want_i)


@pytest.mark.parametrize("name", [c.name for c in T.CASES if c.kind == "merge"])
def test_topk_merge(name):
    c = T.BY_NAME[name]
    _observe(c)
    nshard, kin, kout = c.rows, c.dim, c.k
    d = T.build_merge(name)
    want_s, want_i = T.reference_merge(d["scores"], d["ids"], kout)
    if name == "merge-2x3-10x2":
        assert bool((want_i[:, 4:] == -1).all()) and bool((want_i[:, :4] >= 0).all())            # the generator: padding
    guard_s = torch.full((4096,), NAN32, dtype=torch.int32, device=DEV).view(torch.float32)
    scores = torch.cat([_dev(d["scores"]).reshape(-1), guard_s])
    ids = torch.cat([_dev(d["ids"]).reshape(-1), torch.full((4096,), SENTINEL_ID, dtype=torch.int64, device=DEV)])
    keep = scores.clone(), ids.clone()
    lib = _lib()
    entries = [("uniir_topk_merge_ex", lambda o: lib.uniir_topk_merge_ex(_p(scores), _p(ids), nshard, c.nq, kin, kout, *o.ptrs(), _stream()))]
    if kin == kout:
        entries.append(("uniir_topk_merge", lambda o: lib.uniir_topk_merge(_p(scores), _p(ids), nshard, c.nq, kin, *o.ptrs(), _stream())))
    for what, call in entries:
        def once():
            out = Outputs(c.nq, kout)
            assert call(out) == 0, what
            return out.take()

        res = [once(), _profiled(c, once)]
        assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32)), what
        got_s, got_i = res[0][0].cpu().numpy(), res[0][1].cpu().numpy()
        assert _same_bits(got_s, want_s), (what, np.argwhere(got_s != want_s)[:5])
        assert np.array_equal(got_i, want_i), (what, np.argwhere(got_i != want_i)[:5])
    assert torch.equal(scores.view(torch.int32), keep[0].view(torch.int32)) and torch.equal(ids, keep[1])


def test_the_sweep_loop_equals_the_automatic_width_bit_for_bit():
    """200 queries as sweeps of 64, 64, 64 and 8 (uniir_topk_set_chunk(64), restored whatever happens) against the single sweep"""
    a, b = T.BY_NAME["chunk64-200"], T.BY_NAME["chunk0-200"]
    assert T.build_ip(a.name) is T.build_ip(b.name)
    d = T.build_ip(a.name)
    inp = Inputs(d["pool"], d["ids"], d["queries"])
    lib = _lib()
    assert lib.uniir_topk_set_chunk(64) == 0
    try:
        s64, i64 = _search_ip(a, inp, 0xFF)
    finally:
        assert lib.uniir_topk_set_chunk(0) == 0
    s0, i0 = _search_ip(b, inp, 0xFF)
    assert torch.equal(i64, i0) and torch.equal(s64.view(torch.int32), s0.view(torch.int32))


def test_the_profiler_saw_the_kernels_of_every_case():
    """runs last: the kernel check inside the cases above must not have been empty-handed (a profiler that records nothing would
    let every case pass on whatever kernel ran)"""
    if not SEEN:
        pytest.skip("no case ran before this test")
    if not any(SEEN.values()):
        pytest.skip("the profiler saw none of the library's kernels")
    blind = sorted(n for n, k in SEEN.items() if not k)
    assert not blind, blind
