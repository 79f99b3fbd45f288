"""Case table of the fp16 top-k search suite (test_topk_paths_ref.py on the host, test_topk_paths_gpu.py on the device): a pure-Python
restatement of the host dispatch of csrc/topk.hip and csrc/topk_tail.hip, the cases with the kernel instantiations each is meant to
reach, the numpy generators of their inputs and the references.

The authoritative dispatch table is DESIGN.md "Top-k host layer" (the library's tk_plan implements it); what follows is this
module's own restatement, line for line the rows of that table, which tests/test_topk_refusals_host.py compares with the library's
plan (uniir_topk_plan) for every case here and for shapes too large to run.  It is kept independent on purpose: nothing below
calls the library.

Dispatch restated (one sweep of n <= 1024 queries; ngroups = ceil(rows / 16), kc = k + 8, gcap = 2 kc):
  scan  tk_plan_sweep        n <= 64, dim 768 | 512, rows * dim * 2 < 2^31, ngroups >= 2048   topk_stream2_kernel<dim / 32,2>
                             n <= 64, dim 768 | 512 otherwise                                 topk_stream_kernel<dim / 32>
                             stream_shared_ok: 65 .. 256, dim 768, ngroups >= 2048            topk_stream5_kernel<2 | 4,2> (<= 128 | more)
                             n > 64, dim % 64 == 0, dim >= 192                                topk_gmax_pp_kernel<n <= 128, 2 | 2 | 0>
                             anything else                                                    topk_gmax_kernel<2>   (256-thread selection)
        the two register streaming scans also leave per-wave maxima when ncu * 4 <= 1024 and ceil(ngroups / (ncu * 4)) <= 64
  tail  fused_tail_ok: dim % 64 == 0, dim <= 4096, ngroups even and <= 49152, gcap * 16 <= 2048, behind every scan but the last:
                             topk_tail_select_rescore_kernel<4,3,4 | 2,5,2 | 1,5,2> (n <= 64 | <= 128 | more) + topk_tail_sort_kernel,
                             selection gsel_hier on the wave maxima where the scan left them, else gsel_body<1024,true>
        otherwise launch_select: topk_gsel_kernel<1024,true> (ngroups even, <= 49152), <1024,false> (n <= 64), <256>;
                             uniir_topk_rescore: rescore_coalesced_kernel (dim % 64 == 0) | rescore_kernel, final_sort_kernel by
                             ncand = 32 kc: rank count (<= 1024), registers (<= 2048), re-read loop (more)
  uniir_topk_coarse with more than 1024 queries: topk_coarse_kernel + topk_merge_partial_kernel, ncand = kc
  launch_merge: merge_rank_kernel up to 4096 entries per query, merge_shards_kernel above
  uniir_topk_ip_multi (rows * dim * 2 >= 2^31): equal sub-shards on 32-row boundaries (subshard_rows); batched (multi_batched: one
                             tail, sort and merge launch per sweep for all sub-shards, multi_sweep_path) when every sub-shard, the
                             shorter last one included, is on a register streaming scan and the fused tail in sweeps of <= 256
                             queries and there are <= 64 of them; else one uniir_topk_ip search per sub-shard and one merge
Two branches are taken by the DATA, not the shape; the cases that force them name them as well:
  "gsel_hier bail-out"        more than 128 candidate waves or 1024 groups reach the threshold: gsel_body runs instead
  "gsel_body extraction loop" more than 1024 groups reach the threshold: one extraction per round

References: oracle.c through oracle.c_oracle.topk (the project's pinned chain), queries split over at most 16 host threads; for a
hand-made shortlist the oracle over exactly the live rows; for merges numpy's lexsort on (-score, id) over the live entries.

MASS TIES.  When more groups tie exactly at the k-th best score than the selection keeps (gcap), the search cannot order the tied
rows by id over the whole pool (include/uniir_hip.h [TOPK]).  Only the all-equal-rows pool and the zero query carry `mass_ties` (the
queries concerned); for those queries the answer must be VALID (check_valid_answer), every other query of every case must equal
the oracle in scores and ids."""
import functools
import zlib
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

import numpy as np

TK_G, TK_QT, TK_CT, TK_CAP, TK_MAXKC, TK_GMULT, TK_GPATH_MAXQ = 16, 128, 256, 512, 64, 2, 1024
TK_SELREG, TK_SELCAP, TK_HWAVES, TK_RANKCAP, TKT_SORTCAP, MERGE_CAP, TKI_CHUNK_MAX = 24, 1024, 128, 1024, 2048, 4096, 1024
NCU = 256                       # compute units of the MI355X: the device the cases' named paths are stated for
ORACLE_THREADS = 16
MAX_WORK = 7e9                  # nq * rows * dim of a case: under a second of oracle time on 16 threads


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the host dispatch, restated
def coarse_plan(nq, rows):
    """-> (query tiles, slices, rows per slice)"""
    nqt = cdiv(nq, TK_QT)
    tiles = cdiv(rows, TK_CT)
    want = min(max(cdiv(768, nqt), 1), tiles)
    tps = max(cdiv(tiles, want), 1)
    return nqt, cdiv(rows, tps * TK_CT), tps * TK_CT


def ncand(nq, kc):
    return TK_GMULT * kc * TK_G if nq <= TK_GPATH_MAXQ else kc


def workspace_bytes(nq, kc, rows):
    """uniir_topk_workspace_bytes"""
    if nq <= 0 or kc <= 0 or rows <= 0:
        return 0
    if nq <= TK_GPATH_MAXQ:
        wq = nq if nq <= 256 else 64
        return nq * cdiv(rows, TK_G) * 4 + 256 + max(wq, 64) * 1024 * 4 + 256
    nqt, nsl, _ = coarse_plan(nq, rows)
    return nqt * nsl * TK_QT * TK_CAP * 8 + nsl * nq * kc * 8 + 256


def stream_shared_ok(dim, rows, nq):
    return 64 < nq <= 256 and dim == 768 and rows * 1536 < 2 ** 31 and cdiv(rows, TK_G) >= 2048


def sweep_queries(dim, rows, chunk=0):
    """uniir_topk_ip_sweep_queries under uniir_topk_set_chunk(chunk)"""
    return chunk or (256 if stream_shared_ok(dim, rows, 256) else TKI_CHUNK_MAX)


def ip_workspace_bytes(nq, k, rows, dim, chunk=0):
    """uniir_topk_ip_workspace_bytes_ex"""
    if nq <= 0 or k <= 0 or rows <= 0 or dim <= 0:
        return 0
    c = min(nq, sweep_queries(dim, rows, chunk))
    kc = min(k + 8, TK_MAXKC)
    return workspace_bytes(c, kc, rows) + nq * 4 + 256 + 2 * (c * ncand(c, kc) * 4 + 256)


def wave_maxima(ngroups, ncu):
    return ncu * 4 <= 1024 and cdiv(ngroups, ncu * 4) <= 64


def scan_path(rows, dim, n, ncu):
    """the scan of a sweep -> (kernel, 1 where a 1024-thread selection or the fused tail may follow else 0, per-wave maxima written)"""
    ng = cdiv(rows, TK_G)
    big = dim in (768, 512) and rows * dim * 2 < 2 ** 31 and ng >= 2048
    if n <= 64 and big:
        return f"topk_stream2_kernel<{dim // 32},2>", 1, wave_maxima(ng, ncu)
    if n <= 64 and dim in (768, 512):
        return f"topk_stream_kernel<{dim // 32}>", 1, False
    if stream_shared_ok(dim, rows, n):
        return f"topk_stream5_kernel<{2 if n <= 128 else 4},2>", 1, wave_maxima(ng, ncu)
    if n > 64 and dim % 64 == 0 and dim >= 192:
        return f"topk_gmax_pp_kernel<{'true' if n <= 128 else 'false'},{2 if n <= 256 else 0}>", 1, False
    return "topk_gmax_kernel<2>", 0, False


def fused_tail_ok(rows, dim, kc):
    ng, gcap = cdiv(rows, TK_G), TK_GMULT * kc
    if dim % 64 or dim > 4096 or ng % 2 or ng > 1024 * 2 * TK_SELREG or gcap * TK_G > TKT_SORTCAP or gcap > 2 * TK_MAXKC:
        return False
    return rows * dim * 2 < 2 ** 31


# uniir_topk_ip_multi: a resident shard of >= 2 GiB as equal logical sub-shards
def subshard_rows(rows, dim):
    """uniir_topk_subshard_rows"""
    if rows <= 0 or dim <= 0:
        return 0
    if rows * dim * 2 < 2 ** 31:
        return rows
    cap = min(((2 ** 31 - 1) // (dim * 2)) // 32 * 32, 1024 * 2 * TK_SELREG * TK_G)
    return cdiv(cdiv(rows, cdiv(rows, cap)), 32) * 32


def subshards(rows, dim):
    """-> (rows of a full sub-shard, sub-shards, rows of the last one)"""
    per = subshard_rows(rows, dim)
    nsub = cdiv(rows, per)
    return per, nsub, rows - (nsub - 1) * per


def align256(x):
    return (x + 255) // 256 * 256


def multi_workspace_bytes(nq, k, rows, dim, chunk=0):
    """uniir_topk_ip_multi_workspace_bytes: the larger of the batched layout (per sub-shard: group maxima, wave maxima, candidates,
    exact scores, two k-lists of a sweep) and the per-sub-shard loop's (one uniir_topk_ip workspace + two k-lists of ALL queries per
    sub-shard)"""
    if nq <= 0 or k <= 0 or rows <= 0 or dim <= 0:
        return 0
    if rows * dim * 2 < 2 ** 31:
        return ip_workspace_bytes(nq, k, rows, dim, chunk)
    per, nsub, _ = subshards(rows, dim)
    c = min(nq, sweep_queries(dim, per, chunk))
    g = align256(c * cdiv(per, TK_G) * 4)
    w = align256(max(c if c <= 256 else 64, 64) * 1024 * 4 + 256)
    cb = align256(c * ncand(c, k + 8) * 4)
    o = align256(c * k * 8)
    batched = nsub * (g + w + 2 * cb + 2 * o)
    loop = align256(ip_workspace_bytes(nq, k, per, dim, chunk)) + 2 * nsub * align256(nq * k * 8)
    return max(batched, loop) + 256


def multi_batched(rows, dim, nq, k, chunk=0):
    """does uniir_topk_ip_multi run ONE tail, sort and merge launch per sweep for all sub-shards (else: one uniir_topk_ip per
    sub-shard, one merge)?  Every sub-shard on a register streaming scan and the fused tail, sweeps of <= 256 queries, <= 64 sub-shards"""
    if rows * dim * 2 < 2 ** 31:
        return False
    per, nsub, last = subshards(rows, dim)
    c = min(nq, sweep_queries(dim, per, chunk))
    lg = cdiv(last, TK_G)
    return (dim in (768, 512) and lg >= 2048 and lg % 2 == 0 and c <= 256 and nsub <= 64
            and (c <= 64 or (stream_shared_ok(dim, per, c) and stream_shared_ok(dim, last, c)))
            and fused_tail_ok(per, dim, k + 8) and fused_tail_ok(last, dim, k + 8))


def multi_sweep_path(rows, dim, n, k, ncu):
    """one BATCHED sweep of n queries: the scan of every sub-shard, then one tail for all of them (a workgroup per query, part and
    sub-shard; the hierarchical selection only where every sub-shard's scan leaves wave maxima), one sort, one merge"""
    per, nsub, last = subshards(rows, dim)
    scan, _, _ = scan_path(per, dim, n, ncu)
    assert scan == scan_path(last, dim, n, ncu)[0]
    wm = wave_maxima(cdiv(per, TK_G), ncu) and wave_maxima(cdiv(last, TK_G), ncu)
    parts = "4,3,4" if n * nsub <= 64 else "2,5,2" if n * nsub <= 128 else "1,5,2"
    return (scan, f"topk_tail_select_rescore_kernel<{parts}>", "gsel_hier" if wm else "gsel_body<1024,true>", "topk_tail_sort_kernel",
            "merge_rank_kernel" if nsub * k <= MERGE_CAP else "merge_shards_kernel")


def select_path(sel, rows, n):
    """the stand-alone selection behind a scan (sel: scan_path's second value)"""
    ng = cdiv(rows, TK_G)
    if sel == 1 and ng % 2 == 0 and ng <= 1024 * 2 * TK_SELREG:
        return "topk_gsel_kernel<1024,true>"
    if sel == 1 and n <= 64:
        return "topk_gsel_kernel<1024,false>"
    return "topk_gsel_kernel<256>"


def rescore_path(dim, ncand_):
    """uniir_topk_rescore"""
    branch = "rank" if ncand_ <= TK_RANKCAP else "register" if ncand_ <= 2048 else "reread"
    return ("rescore_coalesced_kernel" if dim % 64 == 0 else "rescore_kernel", f"final_sort_kernel[{branch}]")


def sweep_path(rows, dim, n, k, ncu):
    kc = k + 8
    scan, sel, wm = scan_path(rows, dim, n, ncu)
    if sel >= 1 and fused_tail_ok(rows, dim, kc):
        parts = "4,3,4" if n <= 64 else "2,5,2" if n <= 128 else "1,5,2"      # launch_fused_tail
        return (scan, f"topk_tail_select_rescore_kernel<{parts}>", "gsel_hier" if wm else "gsel_body<1024,true>", "topk_tail_sort_kernel")
    return (scan, select_path(sel, rows, n)) + rescore_path(dim, ncand(n, kc))


def path(rows, dim, nq, k, ncu, chunk=0):
    """the kernels of one uniir_topk_ip call, in first-use order over its sweeps"""
    c = min(nq, sweep_queries(dim, rows, chunk))
    out = []
    for lo in range(0, nq, c):
        for name in sweep_path(rows, dim, min(c, nq - lo), k, ncu):
            if name not in out:
                out.append(name)
    return tuple(out)


def coarse_path(rows, dim, nq, kc, ncu):
    """uniir_topk_coarse"""
    if nq <= TK_GPATH_MAXQ:
        scan, sel, _ = scan_path(rows, dim, nq, ncu)
        return (scan, select_path(sel, rows, nq))
    return ("topk_coarse_kernel", "topk_merge_partial_kernel")


def merge_path(nshard, kin):
    return ("merge_rank_kernel",) if nshard * kin <= MERGE_CAP else ("merge_shards_kernel",)


REQUIRED = (
    "topk_stream_kernel<24>", "topk_stream_kernel<16>", "topk_stream2_kernel<24,2>", "topk_stream2_kernel<16,2>",
    "topk_stream5_kernel<2,2>", "topk_stream5_kernel<4,2>", "topk_gmax_pp_kernel<true,2>", "topk_gmax_pp_kernel<false,2>",
    "topk_gmax_pp_kernel<false,0>", "topk_gmax_kernel<2>", "topk_coarse_kernel", "topk_merge_partial_kernel",
    "topk_gsel_kernel<1024,true>", "topk_gsel_kernel<1024,false>", "topk_gsel_kernel<256>", "gsel_hier", "gsel_body<1024,true>",
    "gsel_hier bail-out", "gsel_body extraction loop",
    "topk_tail_select_rescore_kernel<4,3,4>", "topk_tail_select_rescore_kernel<2,5,2>", "topk_tail_select_rescore_kernel<1,5,2>",
    "topk_tail_sort_kernel", "rescore_kernel", "rescore_coalesced_kernel", "final_sort_kernel[rank]", "final_sort_kernel[register]",
    "final_sort_kernel[reread]", "merge_rank_kernel", "merge_shards_kernel")
DATA_BRANCHES = ("gsel_hier bail-out", "gsel_body extraction loop")

# ------------------------------------------------------------------------------------------------ the cases
# kind "ip": one uniir_topk_ip call.  data: "random" | "fallback" (the planted extraction-loop pool) | "equal" (all rows equal) |
# "zeroq" (query 1 is zero).  mass_ties: the queries whose answer is judged by check_valid_answer.  chunk: uniir_topk_set_chunk.
Case = namedtuple("Case", "name kind reach rows dim nq k data mass_ties chunk")
CASES = []

S1 = {24: "topk_stream_kernel<24>", 16: "topk_stream_kernel<16>"}
S2 = {24: "topk_stream2_kernel<24,2>", 16: "topk_stream2_kernel<16,2>"}
S5_2, S5_4 = "topk_stream5_kernel<2,2>", "topk_stream5_kernel<4,2>"
PP_H, PP_NT, PP_0 = "topk_gmax_pp_kernel<true,2>", "topk_gmax_pp_kernel<false,2>", "topk_gmax_pp_kernel<false,0>"
GMAX = "topk_gmax_kernel<2>"
F4, F2, F1 = (f"topk_tail_select_rescore_kernel<{p}>" for p in ("4,3,4", "2,5,2", "1,5,2"))
BODY, HIER, TSORT = "gsel_body<1024,true>", "gsel_hier", "topk_tail_sort_kernel"
G1024R, G1024, G256 = "topk_gsel_kernel<1024,true>", "topk_gsel_kernel<1024,false>", "topk_gsel_kernel<256>"
RC, RK = "rescore_coalesced_kernel", "rescore_kernel"
FS_RANK, FS_REG, FS_RE = "final_sort_kernel[rank]", "final_sort_kernel[register]", "final_sort_kernel[reread]"


def fused(tail, sel=BODY):
    return (tail, sel, TSORT)


def unfused(sel, sort=FS_RANK, rescore=RC):
    return (sel, rescore, sort)


def ip(name, dim, rows, nq, scan, tail, k=10, data="random", mass_ties=(), chunk=0, extra=()):
    CASES.append(Case(name, "ip", (scan,) + tuple(tail) + tuple(extra), rows, dim, nq, k, data, tuple(mass_ties), chunk))


# queries in LDS (<= 64 queries, fewer than 2048 groups): one row, rows < k, one full group, a ragged second group, an odd and an
# even group count (unfused / fused tail), the last sizes below 2048 groups
for dim, rows, nq in ((768, 1, 1), (512, 5, 7), (768, 16, 64), (768, 33, 7), (512, 33, 64), (768, 4010, 7), (512, 4010, 64),
                      (512, 32752, 7), (768, 32752, 64)):
    ip(f"stream-{dim}-{rows}x{nq}", dim, rows, nq, S1[dim // 32], unfused(G1024))
for dim, rows, nq in ((512, 17, 1), (768, 17, 7), (768, 4000, 64), (512, 4000, 1), (768, 32736, 1), (512, 32736, 64)):
    ip(f"stream-{dim}-{rows}x{nq}", dim, rows, nq, S1[dim // 32], fused(F4))
# queries in registers (>= 2048 groups): exactly 2048 groups with one row in the last, whole groups, an odd count
for dim, rows, nq in ((768, 32753, 1), (768, 32768, 64), (512, 32753, 64), (512, 32768, 33)):
    ip(f"stream2-{dim}-{rows}x{nq}", dim, rows, nq, S2[dim // 32], fused(F4, HIER))
for dim, rows, nq in ((768, 32784, 33), (512, 32784, 1)):
    ip(f"stream2-{dim}-{rows}x{nq}", dim, rows, nq, S2[dim // 32], unfused(G1024))
# the shared-ring scan: 65 .. 128 queries on two waves, 129 .. 256 on four
ip("stream5-32753x65", 768, 32753, 65, S5_2, fused(F2, HIER))
ip("stream5-32768x128", 768, 32768, 128, S5_2, fused(F2, HIER))
ip("stream5-32784x128", 768, 32784, 128, S5_2, unfused(G256))
ip("stream5-32768x129", 768, 32768, 129, S5_4, fused(F1, HIER))
ip("stream5-32753x256", 768, 32753, 256, S5_4, fused(F1, HIER))
ip("stream5-32784x129", 768, 32784, 129, S5_4, unfused(G256))
# the ping-pong scan: half tile (65 .. 128), one tile read once (.. 256), several query tiles; rows around the 256-row tile
ip("pp-192-100x65", 192, 100, 65, PP_H, unfused(G256))
ip("pp-320-256x128", 320, 256, 128, PP_H, fused(F2))
ip("pp-768-4000x128", 768, 4000, 128, PP_H, fused(F2))
ip("pp-512-255x129", 512, 255, 129, PP_NT, fused(F1))
ip("pp-1024-257x256", 1024, 257, 256, PP_NT, unfused(G256))
ip("pp-768-4010x256", 768, 4010, 256, PP_NT, unfused(G256))
ip("pp-768-4000x257", 768, 4000, 257, PP_0, fused(F1))
ip("pp-512-4010x600", 512, 4010, 600, PP_0, unfused(G256))
ip("pp-192-4000x600", 192, 4000, 600, PP_0, fused(F1))
ip("pp-1024-256x1024", 1024, 256, 1024, PP_0, fused(F1))
# the first-generation scan: dims below 192 at any query count, wider ones at <= 64 queries; its selection and the unfused tail
for dim, rows, nq in ((64, 5, 3), (128, 40, 300), (64, 1000, 65), (128, 3001, 64), (192, 1000, 64), (256, 3001, 3), (1024, 40, 64)):
    ip(f"gmax-{dim}-{rows}x{nq}", dim, rows, nq, GMAX, unfused(G256))
ip("gmax-128-1000x1100", 128, 1000, 1100, GMAX, unfused(G256))          # two sweeps: 1024 + 76 queries
# the fused tail's width and depth: 3, 4, 16 and 64 slices of 64 columns taken, 65 refused (register selection + unfused tail)
ip("tail-192-512x65", 192, 512, 65, PP_H, fused(F2))
ip("tail-256-1024x129", 256, 1024, 129, PP_NT, fused(F1))
ip("tail-1024-2048x65", 1024, 2048, 65, PP_H, fused(F2))
ip("tail-4096-512x70", 4096, 512, 70, PP_H, fused(F2))
ip("tail-4160-512x70", 4160, 512, 70, PP_H, unfused(G1024R))
# k = 1; k = 50 (1856 slots: several 512-slot re-score rounds); k = 56 (kc = 64, gcap * 16 == 2048 slots exactly)
ip("k1-fused", 768, 4000, 7, S1[24], fused(F4), k=1)
ip("k1-unfused", 768, 4010, 7, S1[24], unfused(G1024), k=1)
ip("k50-stream2", 768, 32768, 64, S2[24], fused(F4, HIER), k=50)
ip("k50-pp", 512, 4000, 200, PP_NT, fused(F1), k=50)
ip("k56-fused", 768, 4000, 64, S1[24], fused(F4), k=56)
ip("k56-unfused", 768, 4010, 64, S1[24], unfused(G1024, FS_REG), k=56)
ip("k56-gmax", 128, 3001, 65, GMAX, unfused(G256, FS_REG), k=56)
ip("k56-stream5", 768, 32768, 128, S5_2, fused(F2, HIER), k=56)
# the sweep loop: 200 queries as sweeps of 64, 64, 64 and 8; must equal the one sweep of the automatic width bit for bit
ip("chunk64-200", 768, 4000, 200, S1[24], fused(F4), chunk=64)
ip("chunk0-200", 768, 4000, 200, PP_NT, fused(F1))
# adversarial selection, 40 000 x 768 (2500 groups, fused tail): the planted pool drives the hierarchical selection into its
# bail-out and gsel_body into the extraction loop, with an unambiguous top 10; then the two mass ties
for nq, scan, tail in ((2, S2[24], F4), (64, S2[24], F4), (200, S5_4, F1)):
    ip(f"fallback-x{nq}", 768, 40000, nq, scan, fused(tail, HIER), data="fallback", extra=DATA_BRANCHES + (BODY,))
ip("equal-rows", 768, 40000, 3, S2[24], fused(F4, HIER), data="equal", mass_ties=(0, 1, 2), extra=DATA_BRANCHES + (BODY,))
ip("zero-query", 768, 40000, 3, S2[24], fused(F4, HIER), data="zeroq", mass_ties=(1,), extra=DATA_BRANCHES + (BODY,))

# kind "coarse": uniir_topk_coarse + uniir_topk_rescore called one after the other (k = 10, kc = 18)
CASES.append(Case("coarse-1100x3000x128", "coarse", ("topk_coarse_kernel", "topk_merge_partial_kernel", RC, FS_RANK),
                  3000, 128, 1100, 10, "random", (), 0))
CASES.append(Case("coarse-40x1000x96", "coarse", (GMAX, G256, RK, FS_RANK), 1000, 96, 40, 10, "random", (), 0))
# kind "rescore": uniir_topk_rescore alone on a hand-made shortlist of `rows` entries per query (pool of SHORTLIST_POOL rows); data
# "noids": pool_ids == NULL
SHORTLIST_POOL = 3000
for n_, data_, sort_ in ((600, "ids", FS_RANK), (600, "noids", FS_RANK), (1500, "ids", FS_REG), (2500, "ids", FS_RE), (2500, "noids", FS_RE)):
    CASES.append(Case(f"rescore-{n_}-{data_}", "rescore", (RC, sort_), n_, 64, 5, 10, data_, (), 0))
# kind "merge": (nshard, k_in, k_out, nq) as (rows, dim, k, nq); both entry points where k_in == k_out
for ns_, kin_, kout_, nq_ in ((1, 10, 10, 3), (8, 10, 10, 64), (3, 10, 25, 5), (4, 1024, 56, 300), (5, 1024, 56, 300), (2, 3, 10, 2)):
    CASES.append(Case(f"merge-{ns_}x{kin_}-{kout_}x{nq_}", "merge", merge_path(ns_, kin_), ns_, kin_, nq_, kout_, "merge", (), 0))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def case_path(c, ncu):
    """what the host layer launches for the case on a device with ncu compute units (the data-taken branches excluded)"""
    if c.kind == "ip":
        return path(c.rows, c.dim, c.nq, c.k, ncu, c.chunk)
    if c.kind == "coarse":
        kc = c.k + 8
        return coarse_path(c.rows, c.dim, c.nq, kc, ncu) + rescore_path(c.dim, ncand(c.nq, kc))
    if c.kind == "rescore":
        return rescore_path(c.dim, c.rows)
    return merge_path(c.rows, c.dim)


_unreached = [r for r in REQUIRED if not any(r in c.reach for c in CASES)]
assert not _unreached, _unreached
for _c in CASES:
    _named = tuple(r for r in _c.reach if r not in DATA_BRANCHES and not (r == BODY and HIER in _c.reach))
    assert set(case_path(_c, NCU)) == set(_named), (_c.name, case_path(_c, NCU), _named)
    assert set(_c.reach) <= set(REQUIRED), _c.name
    assert _c.kind != "ip" or _c.nq * _c.rows * _c.dim <= MAX_WORK, _c.name
    assert not _c.mass_ties or _c.data in ("equal", "zeroq"), _c.name


# ------------------------------------------------------------------------------------------------ inputs
ZERO_ROW, DUP_SRC = 17, 5            # decorations of every pool of >= 200 rows: a zero row; the LAST row duplicates row DUP_SRC;
#                                      the last query equals the last row (so its two best hits tie exactly and the id decides)
FB_TOP_ROWS = (7 * 16 + 1, 7 * 16 + 5, 7 * 16 + 9, 7 * 16 + 15, 1203 * 16, 1203 * 16 + 2, 1203 * 16 + 3, 2498 * 16 + 4, 2498 * 16 + 14,
               2498 * 16 + 15)       # the fallback pool: ten rows in three groups, cosines 0.90, 0.89 .. 0.81 to query 0
FB_DUP_COS, FB_NDUP = 0.5, 1100      # and one row at cosine 0.5, copied into 1100 other groups


def _seed(name):
    return zlib.crc32(name.encode())


def _with_cos(rng, qn, cos, n):
    noise = rng.standard_normal((n, qn.shape[0]))
    noise -= (noise @ qn)[:, None] * qn[None, :]
    noise /= np.linalg.norm(noise, axis=1, keepdims=True)
    cos = np.broadcast_to(np.asarray(cos, dtype=np.float64), (n,))
    return cos[:, None] * qn[None, :] + np.sqrt(1 - cos * cos)[:, None] * noise


def fallback_dup_rows(rng, rows):
    """one row in each of FB_NDUP groups spread over the pool, none in a group that holds a planted or decorated row"""
    ng = rows // TK_G
    taken = {r // TK_G for r in FB_TOP_ROWS} | {ZERO_ROW // TK_G, DUP_SRC // TK_G, (rows - 1) // TK_G}
    free = np.array([g for g in range(ng) if g not in taken])
    groups = np.sort(rng.choice(free, FB_NDUP, replace=False))
    return groups * TK_G + (groups * 7) % TK_G


DATA_OF = {"chunk64-200": "chunk0-200"}        # the two sweep-loop cases share their inputs (and their reference)


def build_ip(name):
    """-> dict(pool fp16 [rows][dim], ids int64 [rows], queries fp16 [nq][dim]) (+ dup_rows for the fallback pool); read-only"""
    return _build_ip(DATA_OF.get(name, name))


@functools.lru_cache(maxsize=3)
def _build_ip(name):
    c = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    out = {}
    if c.data == "equal":
        pool = np.repeat(rng.standard_normal((1, c.dim)).astype(np.float16), c.rows, axis=0)
        queries = rng.standard_normal((c.nq, c.dim)).astype(np.float16)
    else:
        pool = rng.standard_normal((c.rows, c.dim), dtype=np.float32)
        queries = rng.standard_normal((c.nq, c.dim), dtype=np.float32)
        if c.data == "fallback":
            pool *= 0.3
            qn = queries[0].astype(np.float64)
            qn /= np.linalg.norm(qn)
            scale = 1.0 + 0.1 * np.arange(10)
            pool[list(FB_TOP_ROWS)] = _with_cos(rng, qn, 0.90 - 0.01 * np.arange(10), 10) * scale[:, None]
            out["dup_rows"] = fallback_dup_rows(rng, c.rows)
            pool[out["dup_rows"]] = _with_cos(rng, qn, FB_DUP_COS, 1).astype(np.float16)
        pool, queries = pool.astype(np.float16), queries.astype(np.float16)
        if c.rows >= 200:
            pool[ZERO_ROW] = 0
            pool[c.rows - 1] = pool[DUP_SRC]
            queries[c.nq - 1] = pool[c.rows - 1]
        if c.data == "zeroq":
            queries[1] = 0
    ids = (rng.permutation(c.rows) * 5 + 123).astype(np.int64)
    out.update(pool=pool, ids=ids, queries=queries)
    for v in out.values():
        v.setflags(write=False)
    return out


def shortlist_pairs(ncand):
    """(query, row, position of the copy with the LARGER id, position of the other): exact ties planted at the top of three
    shortlists.  Positions 256 apart belong to one thread of final_sort_kernel (entry c sits in thread c % 256), the larger id
    first, so a sort that does not let the id decide inside a thread's own entries gets them wrong; the second pair lies in the
    part of a long shortlist that is re-read every round (c >= 2048); the third at both ends."""
    return ((0, 1, 3, 259), (1, 2, 2100, 2356) if ncand > 2356 else (1, 2, 40, 41), (2, 3, 0, ncand - 1))


def build_shortlists(name):
    """hand-made shortlists for uniir_topk_rescore alone: unique rows per query, a third of the entries -1, duplicate pool rows
    (r and r + 1500) among them, planted ties (shortlist_pairs), query 3 with fewer live entries than k
    -> dict(pool, ids | None, queries, cand int32 [nq][ncand])"""
    c = BY_NAME[name]
    rng = np.random.default_rng(_seed(name))
    pool = rng.standard_normal((SHORTLIST_POOL, c.dim)).astype(np.float16)
    pool[1500:2500] = pool[:1000]                      # exact duplicates 1500 rows apart: most shortlists hold both of a pair
    pool[ZERO_ROW] = 0
    queries = rng.standard_normal((c.nq, c.dim)).astype(np.float16)
    ids = None if c.data == "noids" else (rng.permutation(SHORTLIST_POOL) * 5 + 123).astype(np.int64)
    cand = np.stack([rng.permutation(SHORTLIST_POOL)[:c.rows] for _ in range(c.nq)]).astype(np.int32)
    dead = rng.random(cand.shape) < 1.0 / 3.0
    for q, r, p_hi, p_lo in shortlist_pairs(c.rows):
        queries[q] = pool[r]
        rest = rng.permutation(SHORTLIST_POOL)
        cand[q] = rest[~np.isin(rest, (r, r + 1500))][:c.rows]
        hi, lo = (r + 1500, r) if ids is None or ids[r + 1500] > ids[r] else (r, r + 1500)
        cand[q, p_hi], cand[q, p_lo] = hi, lo
        dead[q, p_hi] = dead[q, p_lo] = False
    cand[dead] = -1
    cand[3, 4:] = -1                                   # at most 4 live entries: the rest of the k results is padding
    cand[3, 1] = cand[3, 1] if cand[3, 1] >= 0 else 7
    return dict(pool=pool, ids=ids, queries=queries, cand=cand)


def build_merge(name):
    """per-shard lists [nshard][nq][k_in] (score desc, -inf / -1 tails), scores from a coarse grid so that they tie across shards,
    ids unique, shard 1 empty (where there are more than two)"""
    c = BY_NAME[name]
    nshard, kin, nq = c.rows, c.dim, c.nq
    rng = np.random.default_rng(_seed(name))
    scores = -np.sort(-(rng.integers(0, 512, (nshard, nq, kin)) / np.float32(64)).astype(np.float32), axis=2)
    ids = (rng.permutation(nshard * nq * kin).reshape(nshard, nq, kin) * 3 + 11).astype(np.int64)
    live = rng.integers(0, kin + 1, (nshard, nq))
    live[0, :] = kin if nshard * kin >= c.k else live[0, :]
    if name == "merge-2x3-10x2":
        live[:] = 2                                    # 4 live entries < k_out = 10
    if nshard > 2:
        live[1, :] = 0
    dead = np.arange(kin)[None, None, :] >= live[:, :, None]
    scores[dead], ids[dead] = -np.inf, -1
    return dict(scores=scores, ids=ids)


# ------------------------------------------------------------------------------------------------ references
def oracle_topk_mt(pool, ids, queries, k):
    """oracle.c top-k, the queries split over at most ORACLE_THREADS host threads (ctypes releases the GIL)"""
    from oracle import c_oracle
    nthr = max(1, min(ORACLE_THREADS, queries.shape[0]))
    parts = np.array_split(np.arange(queries.shape[0]), nthr)
    with ThreadPoolExecutor(nthr) as ex:
        outs = list(ex.map(lambda idx: c_oracle.topk(pool, ids, queries[idx], k), parts))
    return np.concatenate([o[0] for o in outs]), np.concatenate([o[1] for o in outs])


@functools.lru_cache(maxsize=4)
def _reference_ip(name):
    d = _build_ip(name)
    s, i = oracle_topk_mt(d["pool"], d["ids"], d["queries"], BY_NAME[name].k + 1)
    s.setflags(write=False)
    i.setflags(write=False)
    return s, i


def reference_ip(name):
    """the oracle's top k + 1 of an "ip" / "coarse" case (the first k columns are its top k); computed once per input set"""
    return _reference_ip(DATA_OF.get(name, name))


def reference_shortlist(d, k):
    """the oracle's score of exactly the live rows of each shortlist, ordered by (score desc, id asc), (-inf, -1) padded"""
    from oracle import c_oracle
    nq = d["queries"].shape[0]
    s, i = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
    for q in range(nq):
        rows = d["cand"][q][d["cand"][q] >= 0].astype(np.int64)
        sub_ids = rows if d["ids"] is None else d["ids"][rows]
        s[q], i[q] = (x[0] for x in c_oracle.topk(d["pool"][rows], sub_ids, d["queries"][q:q + 1], k))
    return s, i


def reference_merge(scores, ids, k):
    nshard, nq, kin = scores.shape
    s, i = np.full((nq, k), -np.inf, np.float32), np.full((nq, k), -1, np.int64)
    for q in range(nq):
        fs, fi = scores[:, q, :].reshape(-1), ids[:, q, :].reshape(-1)
        fs, fi = fs[fi >= 0], fi[fi >= 0]
        order = np.lexsort((fi, -fs))[:k]
        s[q, :len(order)], i[q, :len(order)] = fs[order], fi[order]
    return s, i


def check_valid_answer(pool, ids, query, k, got_s, got_i, want_s):
    """the contract of a mass-tied query: None when (got_s, got_i) is a valid answer, else what is wrong with it.
    Scores bit-equal to the oracle's at every rank; ids distinct, >= 0 and of the pool; the oracle's own score of every returned
    (query, id) pair is the returned score, bit for bit; among equal scores the ids ascend."""
    from oracle import c_oracle
    if got_s.view(np.uint32).tolist() != np.asarray(want_s, np.float32).view(np.uint32).tolist():
        return "scores differ from the oracle's"
    n = min(k, pool.shape[0])
    if (got_i[n:] != -1).any():
        return "padding ids"
    live = got_i[:n]
    if (live < 0).any() or len(set(live.tolist())) != n:
        return "ids negative or repeated"
    order = np.argsort(ids, kind="stable")
    pos = np.searchsorted(ids, live, sorter=order)
    if (pos >= len(ids)).any() or (ids[order[np.minimum(pos, len(ids) - 1)]] != live).any():
        return "an id that is not in the pool"
    rows = order[pos]
    s, i = c_oracle.topk(pool[rows], ids[rows], query[None, :], n)      # the oracle over exactly the returned rows: its order is
    if s[0].view(np.uint32).tolist() != got_s[:n].view(np.uint32).tolist():   # (score desc, id asc), so both lists must match
        return "a returned score is not the oracle's score of that row"
    if i[0].tolist() != live.tolist():
        return "ids do not ascend among equal scores"
    return None
