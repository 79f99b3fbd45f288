"""Host-side checks of tests/topk_cases.py (no GPU).  Importing the module already asserts that every instantiation is named by a
case and that path() of every case at 256 compute units yields what the case names; here: the planted structures have the
properties the device cases rely on, the generators give what they promise, and the validity checker of the mass-tied queries
accepts a right answer and rejects a wrong one."""
import numpy as np
import pytest

import topk_cases as T

FALLBACK = [c.name for c in T.CASES if c.data == "fallback"]
FLAGGED = [c.name for c in T.CASES if c.mass_ties]
NW, BS = 1024, 1024


def _exact_group_maxima(d, q):
    """the oracle's score of every row against query q, as group maxima"""
    rows = d["pool"].shape[0]
    s, i = T.oracle_topk_mt(d["pool"], np.arange(rows, dtype=np.int64), d["queries"][q:q + 1], rows)
    score = np.empty(rows, np.float32)
    score[i[0]] = s[0]
    return score.reshape(-1, T.TK_G).max(axis=1), score


def test_every_required_instantiation_is_named_and_nothing_else():
    assert not [r for r in T.REQUIRED if not any(r in c.reach for c in T.CASES)]
    assert sorted({c.name for c in T.CASES if c.mass_ties}) == ["equal-rows", "zero-query"]
    for c in T.CASES:
        assert c.kind != "ip" or c.k == 10 or c.name.startswith(("k1-", "k50-", "k56-")), c.name


def test_path_changes_where_the_host_layer_does():
    """each side of every threshold of the restated dispatch"""
    P = lambda *a: T.path(*a, T.NCU)          # noqa: E731
    assert P(32752, 768, 64, 10)[0] == "topk_stream_kernel<24>" and P(32753, 768, 64, 10)[0] == "topk_stream2_kernel<24,2>"
    assert P(32753, 768, 65, 10)[0] == "topk_stream5_kernel<2,2>" and P(32752, 768, 65, 10)[0] == "topk_gmax_pp_kernel<true,2>"
    assert P(32768, 768, 128, 10)[0] == "topk_stream5_kernel<2,2>" and P(32768, 768, 129, 10)[0] == "topk_stream5_kernel<4,2>"
    assert P(32768, 512, 65, 10)[0] == "topk_gmax_pp_kernel<true,2>"
    assert P(4000, 192, 65, 10)[0] == "topk_gmax_pp_kernel<true,2>" and P(4000, 128, 65, 10)[0] == "topk_gmax_kernel<2>"
    assert P(4000, 192, 64, 10)[0] == "topk_gmax_kernel<2>"
    assert P(4000, 256, 256, 10)[0] == "topk_gmax_pp_kernel<false,2>" and P(4000, 256, 257, 10)[0] == "topk_gmax_pp_kernel<false,0>"
    assert "topk_tail_select_rescore_kernel<4,3,4>" in P(4000, 768, 64, 10) and "topk_tail_select_rescore_kernel<2,5,2>" in P(4000, 768, 65, 10)
    assert "topk_tail_select_rescore_kernel<2,5,2>" in P(4000, 768, 128, 10) and "topk_tail_select_rescore_kernel<1,5,2>" in P(4000, 768, 129, 10)
    assert T.fused_tail_ok(512, 4096, 18) and not T.fused_tail_ok(512, 4160, 18) and not T.fused_tail_ok(4010, 768, 18)
    assert T.fused_tail_ok(4000, 768, 64) and not T.fused_tail_ok(4000, 768, 65)
    assert T.fused_tail_ok(786432, 768, 18) and not T.fused_tail_ok(786464, 768, 18)
    assert T.rescore_path(768, 1024)[1].endswith("[rank]") and T.rescore_path(768, 1056)[1].endswith("[register]")
    assert T.rescore_path(768, 2048)[1].endswith("[register]") and T.rescore_path(768, 2049)[1].endswith("[reread]")
    assert T.rescore_path(96, 576)[0] == "rescore_kernel"
    assert T.merge_path(4, 1024) == ("merge_rank_kernel",) and T.merge_path(5, 1024) == ("merge_shards_kernel",)
    assert T.wave_maxima(2048, 256) and not T.wave_maxima(2048, 304) and T.wave_maxima(65536, 256) and not T.wave_maxima(65537, 256)
    # more than 256 queries of a dim-768 shard with >= 2048 groups are swept 256 at a time; other shapes 1024 at a time
    assert T.path(40000, 768, 300, 10, T.NCU)[0] == "topk_stream5_kernel<4,2>" and "topk_stream2_kernel<24,2>" in T.path(40000, 768, 300, 10, T.NCU)
    assert T.coarse_path(3000, 128, 1024, 18, T.NCU)[0] == "topk_gmax_kernel<2>" and T.coarse_path(3000, 128, 1025, 18, T.NCU)[0] == "topk_coarse_kernel"


@pytest.mark.parametrize("name", FALLBACK)
def test_the_planted_pool_forces_the_fallbacks(name):
    c = T.BY_NAME[name]
    d = T.build_ip(name)
    ng = T.cdiv(c.rows, T.TK_G)
    assert ng % 2 == 0 and T.fused_tail_ok(c.rows, c.dim, c.k + 8)
    gm, score = _exact_group_maxima(d, 0)
    dup_level = float(score[d["dup_rows"][0]])
    assert abs(dup_level - T.FB_DUP_COS) < 2e-3 and np.all(score[d["dup_rows"]] == score[d["dup_rows"][0]])
    # the ten best rows are the planted ones, in three groups, well above the copies; everything else lies below the copies
    top = np.argsort(-score, kind="stable")[:10]
    assert sorted(top.tolist()) == sorted(T.FB_TOP_ROWS) and len({r // T.TK_G for r in T.FB_TOP_ROWS}) == 3
    assert score[top].min() > 0.8 and np.all(np.diff(np.sort(score[top])) > 5e-3)
    others = np.ones(c.rows, bool)
    others[list(T.FB_TOP_ROWS)] = False
    others[d["dup_rows"]] = False
    assert score[others].max() < dup_level - 0.1
    # gsel_body<1024, REG>: thread t holds groups 2 (it * 1024 + t) + h, a quarter wave is 16 threads -> 64 interleaved clusters; the
    # threshold is the k-th largest cluster maximum, so with at most nine clusters above the copies it falls to their level
    groups = np.arange(ng)
    cluster = ((groups // 2) % BS) // 16
    cmax = np.array([gm[cluster == j].max() for j in range(64)])
    assert (cmax > dup_level).sum() <= 9 and (cmax >= dup_level).sum() >= c.k
    # ... and more than TK_SELCAP groups reach it: the collection overflows into the extraction loop (the scan's rounding error
    # is far below the 0.1 that separates the copies from everything under them)
    assert (gm >= dup_level).sum() == T.FB_NDUP + 3 > T.TK_SELCAP
    # gsel_hier: the same threshold from the wave maxima (wave w owns groups [w ng / nw, (w + 1) ng / nw)); the copies span more
    # than TK_HWAVES wave ranges, so it bails out first
    wave_of = np.searchsorted(np.arange(1, NW + 1) * ng // NW, groups, side="right")
    assert all(w * ng // NW <= g < (w + 1) * ng // NW for g, w in zip(groups[::97], wave_of[::97]))
    wmax = np.array([gm[wave_of == w].max() if (wave_of == w).any() else -np.inf for w in range(NW)])
    qmax = wmax.reshape(64, 16).max(axis=1)
    assert (qmax > dup_level).sum() <= 9
    assert len(set(wave_of[d["dup_rows"] // T.TK_G].tolist())) > T.TK_HWAVES
    # no other query of the case meets the copies among its best k + 1 (that would be a mass tie of its own)
    ref_s, ref_i = T.reference_ip(name)
    dup_ids = set(d["ids"][d["dup_rows"]].tolist())
    assert not any(dup_ids & set(ref_i[q].tolist()) for q in range(1, c.nq))


@pytest.mark.parametrize("name", [c.name for c in T.CASES if c.kind in ("ip", "coarse") and not c.mass_ties])
def test_the_oracles_kth_and_next_entry_differ(name):
    """guards the generator: the reference's (score, id) pairs at ranks k and k + 1 are distinct, ids are unique, the decorations
    are in place"""
    c = T.BY_NAME[name]
    d = T.build_ip(name)
    assert len(np.unique(d["ids"])) == c.rows and d["pool"].dtype == np.float16 and d["queries"].shape == (c.nq, c.dim)
    if c.rows >= 200:
        assert not d["pool"][T.ZERO_ROW].any() and np.array_equal(d["pool"][c.rows - 1], d["pool"][T.DUP_SRC])
        assert np.array_equal(d["queries"][c.nq - 1], d["pool"][c.rows - 1])
    s, i = T.reference_ip(name)
    assert s.shape == (c.nq, c.k + 1)
    if c.rows > c.k:
        assert np.all((s[:, c.k - 1] != s[:, c.k]) | (i[:, c.k - 1] != i[:, c.k]))
        assert np.all(s[:, :-1] >= s[:, 1:])
    else:
        assert np.all(i[:, c.rows:] == -1) and np.all(np.isneginf(s[:, c.rows:]))
    if c.rows >= 200:         # the last query's two best hits are the duplicate pair, in id order
        pair = sorted(d["ids"][[T.DUP_SRC, c.rows - 1]].tolist())
        assert i[c.nq - 1, :2].tolist() == pair
        assert s[c.nq - 1, 0] == s[c.nq - 1, 1]


@pytest.mark.parametrize("name", FLAGGED)
def test_the_validity_checker_accepts_the_oracle_and_rejects_a_foreign_row(name):
    c = T.BY_NAME[name]
    d = T.build_ip(name)
    s, i = T.reference_ip(name)
    for q in c.mass_ties:
        ws, wi = np.ascontiguousarray(s[q, :c.k]), np.ascontiguousarray(i[q, :c.k])
        assert ws[0] == ws[-1] == s[q, c.k], "not a mass tie"
        assert T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], c.k, ws, wi, ws) is None
        # another valid answer: tied rows from the far end of the pool, ids ascending
        if c.data == "equal":
            far = np.sort(d["ids"][-c.k:])
            assert T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], c.k, ws, far, ws) is None
            # ... in descending order it is not
            assert T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], c.k, ws, far[::-1].copy(), ws) is not None
        bad = wi.copy()
        bad[3] = bad[2]
        assert T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], c.k, ws, bad, ws) is not None          # a repeated id
        bad = wi.copy()
        bad[3] = 7                                                                                              # no id of the pool
        assert 7 not in d["ids"] and T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], c.k, ws, bad, ws) is not None
        bad_s = ws.copy()
        bad_s[0] = np.nextafter(bad_s[0], np.float32(2))
        assert T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], c.k, bad_s, wi, ws) is not None
    # one id swapped for a row that does NOT tie: a query whose scores differ from row to row
    q = [x for x in range(c.nq) if x not in c.mass_ties]
    if q:
        q = q[0]
        ws, wi = np.ascontiguousarray(s[q, :c.k]), np.ascontiguousarray(i[q, :c.k])
        assert T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], c.k, ws, wi, ws) is None
        bad = wi.copy()
        bad[4] = i[q, c.k]                      # the (k + 1)-th entry: a real row, but not one with that score
        assert s[q, c.k] != s[q, 4]
        assert T.check_valid_answer(d["pool"], d["ids"], d["queries"][q], c.k, ws, bad, ws) is not None
    else:                                       # all rows tie for every query: swap in a row of ANOTHER pool by changing the query
        other = (d["queries"][0].astype(np.float32) * np.float32(-1)).astype(np.float16)
        ws, wi = np.ascontiguousarray(s[0, :c.k]), np.ascontiguousarray(i[0, :c.k])
        assert T.check_valid_answer(d["pool"], d["ids"], other, c.k, ws, wi, ws) is not None


@pytest.mark.parametrize("name", [c.name for c in T.CASES if c.kind == "rescore"])
def test_the_hand_made_shortlists_hold_what_they_promise(name):
    c = T.BY_NAME[name]
    d = T.build_shortlists(name)
    cand = d["cand"]
    assert cand.shape == (c.nq, c.rows) and cand.max() < T.SHORTLIST_POOL
    for q in range(c.nq):
        live = cand[q][cand[q] >= 0]
        assert len(set(live.tolist())) == len(live)                       # a row at most once per shortlist
    dead = (cand < 0).mean()
    assert 0.25 < (cand[[0, 1, 2, 4]] < 0).mean() < 0.42, dead
    assert 0 < (cand[3] >= 0).sum() < c.k
    both = set(cand[1][cand[1] >= 0].tolist())
    assert sum(1 for r in both if r < 1000 and r + 1500 in both) >= 10    # duplicate pool rows inside one shortlist
    assert (d["ids"] is None) == (c.data == "noids")
    s, i = T.reference_shortlist(d, c.k)
    for q, r, p_hi, p_lo in T.shortlist_pairs(c.rows):                    # the planted exact ties are decided by the id
        want = {r, r + 1500} if d["ids"] is None else {int(d["ids"][r]), int(d["ids"][r + 1500])}
        assert s[q, 0] == s[q, 1] > s[q, 2] and i[q, 0] < i[q, 1] and {int(i[q, 0]), int(i[q, 1])} == want
        assert {int(cand[q, p_hi]), int(cand[q, p_lo])} == {r, r + 1500} and p_hi < p_lo < c.rows
        id_of = (lambda x: x) if d["ids"] is None else (lambda x: int(d["ids"][x]))
        assert id_of(int(cand[q, p_hi])) > id_of(int(cand[q, p_lo]))          # the larger id comes first
    q, r, p_hi, p_lo = T.shortlist_pairs(c.rows)[0]
    assert p_hi % 256 == p_lo % 256 and p_lo < 2048                       # one thread's registers hold both
    if c.rows > 2048:
        q, r, p_hi, p_lo = T.shortlist_pairs(c.rows)[1]
        assert p_hi % 256 == p_lo % 256 and p_hi >= 2048                  # the re-read part, the same thread


@pytest.mark.parametrize("name", [c.name for c in T.CASES if c.kind == "merge"])
def test_the_merge_inputs_hold_what_they_promise(name):
    c = T.BY_NAME[name]
    d = T.build_merge(name)
    s, i = d["scores"], d["ids"]
    live = i >= 0
    assert len(np.unique(i[live])) == live.sum() and np.all(np.isneginf(s[~live]))
    assert np.all(live[:, :, :-1] >= live[:, :, 1:])                      # -1 entries only at the tails
    if c.rows > 2:
        assert not live[1].any()                                          # an empty shard
        assert len(np.unique(s[live])) < live.sum()                       # equal scores
    ws, wi = T.reference_merge(s, i, c.k)
    assert ws.shape == (c.nq, c.k) and np.all(ws[:, :-1] >= ws[:, 1:])
    if name == "merge-2x3-10x2":
        assert np.all(wi[:, 4:] == -1) and np.all(wi[:, :4] >= 0)
    if name == "merge-8x10-10x64":        # equal scores across shards inside the answer, ids ascending among them
        ties = (ws[:, :-1] == ws[:, 1:]) & (wi[:, 1:] >= 0)
        assert ties.any() and np.all(wi[:, :-1][ties] < wi[:, 1:][ties])
