"""The fp32 candidate-pool search (uniir_topk_ip_f32 through uniir_amd.retrieval) on the device: bit for bit the fp16 search on
fp16-representable rows, bit for bit tests/topk_f32_ref.py (the numpy restatement of the contract) on genuine fp32 rows."""
import functools

import numpy as np
import pytest
import torch

import topk_f32_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _same(got, want):
    s, i = got
    ws, wi = want
    return np.array_equal(i.cpu().numpy(), wi) and np.array_equal(s.cpu().numpy(), ws)


def _plant(pool, rng):
    """a zero row, duplicates (the last row of the ragged last group among them), and -- on pools large enough -- a few hundred rows
    scaled far out of fp16's range in both directions"""
    n = pool.shape[0]
    if n >= 1000:
        pool[3:n:37][:300] *= np.float32(1e-4)
        pool[5:n:41][:300] *= np.float32(3e4)
        pool[n // 3] = 0
        pool[n // 2] = pool[7]
        pool[n - 1] = pool[7]
    return pool


@functools.lru_cache(maxsize=None)
def _f32_case(n, nq, dim, k):
    """genuine fp32 rows, permuted ids, and the restatement's answer (computed once per shape)"""
    rng = np.random.default_rng(n * 31 + nq * 7 + dim + k)
    pool = _plant((rng.standard_normal((n, dim)) * 0.3).astype(np.float32), rng)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) * 3 + 5
    return pool, ids, q, R.topk(pool, ids, q, k)


def _shard(pool, ids):
    from uniir_amd import retrieval
    return retrieval.PoolShard(torch.from_numpy(pool).to(DEV), torch.from_numpy(ids).to(DEV))


@pytest.mark.parametrize("n,nq,dim,k", [(40030, 64, 768, 10), (65536, 200, 768, 24), (40030, 64, 512, 50)])
def test_fp16_representable_rows_equal_the_fp16_search(n, nq, dim, k):
    """PoolShard(pool16.float()) searched with q16.float() = PoolShard(pool16) searched with q16: ties the fp32 path to the
    oracle-pinned fp16 one"""
    from uniir_amd import retrieval
    g = torch.Generator(device=DEV).manual_seed(n + nq + dim)
    pool16 = (torch.randn(n, dim, device=DEV, generator=g) * 0.3).half()
    pool16[n // 3] = 0
    pool16[n // 2] = pool16[7]
    pool16[n - 1] = pool16[7]                    # the last row of the ragged last group (40030 = 2501 * 16 + 14)
    q16 = torch.randn(nq, dim, device=DEV, generator=g).half()
    ids = torch.randperm(n, device=DEV, generator=g).to(torch.int64) * 2 + 9
    s16, i16 = retrieval.search_shard(retrieval.PoolShard(pool16, ids), q16, k)
    s32, i32 = retrieval.search_shard(retrieval.PoolShard(pool16.float(), ids), q16.float(), k)
    assert torch.equal(i32, i16) and torch.equal(s32, s16)


@pytest.mark.parametrize("n,nq,dim,k", [(1000, 7, 64, 10), (5, 3, 64, 10), (40030, 64, 768, 10), (40003, 37, 768, 10),
                                        (12000, 300, 768, 50), (9000, 130, 512, 10), (3000, 2300, 256, 10),
                                        (9000, 16, 768, 10), (9000, 17, 768, 10), (9000, 32, 768, 10), (9000, 33, 768, 10),
                                        (9000, 65, 768, 10)])
def test_fp32_rows_equal_the_restatement(n, nq, dim, k):
    """padding (5 rows), a ragged last group (40030), an odd group count (40003), several query tiles, more than one sweep (2300),
    both sides of every query-tile threshold of the scan (16, 32, 64 queries), rows scaled by 1e-4 and 3e4: the scan may not depend on
    fp16's range"""
    from uniir_amd import retrieval
    pool, ids, q, want = _f32_case(n, nq, dim, k)
    got = retrieval.search_shard(_shard(pool, ids), torch.from_numpy(q).to(DEV), k)
    assert _same(got, want)


def test_sweep_loop_with_a_small_chunk():
    """uniir_topk_set_chunk drives the fp32 sweep loop too: 200 queries in sweeps of 64 (the last one of 8)"""
    from uniir_amd import _lib, retrieval
    pool, ids, q, want = _f32_case(40030, 200, 768, 10)
    lib = _lib.load()
    try:
        assert lib.uniir_topk_set_chunk(64) == 0
        got = retrieval.search_shard(_shard(pool, ids), torch.from_numpy(q).to(DEV), 10)
        torch.cuda.synchronize()
    finally:
        assert lib.uniir_topk_set_chunk(0) == 0
    assert _same(got, want)


def _slack(dim):
    """csrc/topk_select.h tk_slack_cos_f32"""
    return max(5.0e-4, 1.78 * 2.0 * (2 * dim + 3) * 1.001 * 2.0 ** -24)


_SPREADS = [0.0, 1e-7, 1e-6, 1e-5, 2e-4, 2e-3, 0.8 * _slack(768), 1.25 * _slack(768)]


@pytest.mark.parametrize("spread", _SPREADS)
@pytest.mark.parametrize("nq", [8, 64])
def test_near_ties_inside_and_around_the_slack(nq, spread):
    """30 rows, each alone in its own 16-row group, whose cosines with a query step by `spread` from 0.9 (the clusters of
    test_topk_candidate_bound_against_adversarial_near_ties): inside the scan's rounding error the approximate ranking is noise and
    every one of them must be re-scored; the device equals the restatement bit for bit.  For spread <= 1e-6 the same rows rounded
    to fp16 rank differently (asserted on the references alone): the search really ran on fp32 rows."""
    from oracle import c_oracle
    from uniir_amd import retrieval
    n, d, k, ncl = 16_000, 768, 10, 8
    rng = np.random.default_rng(int(round(spread * 1e8)) + nq)
    pool = rng.standard_normal((n, d)) * 0.3
    q = rng.standard_normal((nq, d))
    qn = q / np.linalg.norm(q, axis=1, keepdims=True)
    groups = rng.permutation(n // 16 - 1)[:30] * 16 + 3
    for qi in range(ncl):
        rows = (groups + qi) % n
        noise = rng.standard_normal((30, d))
        noise -= (noise @ qn[qi])[:, None] * qn[qi][None, :]
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        cos = 0.9 - spread * np.arange(30)
        pool[rows] = (cos[:, None] * qn[qi][None, :] + np.sqrt(1 - cos * cos)[:, None] * noise) * (1.0 + 0.1 * qi)
    pool, q = pool.astype(np.float32), q.astype(np.float32)
    ids = rng.permutation(n).astype(np.int64) + 11
    want = R.topk(pool, ids, q, k)
    if spread <= 1e-6:
        _, i16 = c_oracle.topk(pool.astype(np.float16), ids, q[:ncl].astype(np.float16), k)
        assert any(not np.array_equal(i16[c], want[1][c]) for c in range(ncl)), "the fp16 pool ranks like the fp32 one: no evidence"
    got = retrieval.search_shard(_shard(pool, ids), torch.from_numpy(q).to(DEV), k)
    assert _same(got, want)


def test_uneven_shards_merged_and_the_subshard_host_loop(monkeypatch):
    from uniir_amd import retrieval
    rng = np.random.default_rng(40)
    n, nq, d, k = 40_000, 33, 768, 10
    pool = _plant((rng.standard_normal((n, d)) * 0.3).astype(np.float32), rng)
    ids = rng.permutation(n).astype(np.int64) + 1
    q = torch.from_numpy(rng.standard_normal((nq, d)).astype(np.float32)).to(DEV)
    full = _shard(pool, ids)
    s, i = retrieval.search_shard(full, q, k)
    cuts = [(0, 13_000), (13_000, 22_001), (22_001, n)]
    res = [retrieval.search_shard(_shard(pool[lo:hi], ids[lo:hi]), q, k) for lo, hi in cuts]
    ms, mi = retrieval.merge_shards(torch.stack([r[0] for r in res]), torch.stack([r[1] for r in res]))
    assert torch.equal(mi, i) and torch.equal(ms, s)
    monkeypatch.setattr(retrieval, "SUBSHARD_BYTES", 1 << 24)
    assert len(retrieval.subshard_bounds(n, d, 4)) > 2
    ss, si = retrieval.search_shard(full, q, k)
    assert torch.equal(si, i) and torch.equal(ss, s)


@pytest.mark.parametrize("n", [3000, 40])
def test_large_k_through_slices(n):
    from uniir_amd import retrieval
    pool, ids, q, want = _f32_case(n, 5, 64, 100)
    got = retrieval.search_shard(_shard(pool, ids), torch.from_numpy(q).to(DEV), 100)
    assert _same(got, want)
    if n == 40:
        assert np.all(want[1][:, 40:] == -1)


def test_embed_resident_keeps_fp32_rows_and_search_resident_searches_them():
    from uniir_amd import retrieval
    g = torch.Generator().manual_seed(3)
    table = torch.randn(500, 128, generator=g)

    class Fake(torch.nn.Module):
        def forward(self, batch, encode_mbeir_batch=False):
            assert encode_mbeir_batch and batch["x"].is_cuda
            return batch["x"] * 1.5, batch["did_list"]

    def loader():
        return [{"x": table[lo:lo + 64], "did_list": list(range(9_000_001 + lo, 9_000_001 + min(500, lo + 64)))}
                for lo in range(0, 500, 64)]

    emb, ids = retrieval.embed_resident(Fake(), loader(), torch.device("cuda"), dtype=torch.float32)
    assert emb.dtype == torch.float32 and emb.is_cuda and emb.shape == (500, 128) and ids.dtype == torch.int64
    assert torch.equal(emb.cpu(), table * 1.5)
    shard = retrieval.PoolShard(emb, ids)
    assert shard.emb.dtype == torch.float32
    queries = torch.randn(21, 128, generator=g).cuda()
    got = retrieval.search_resident(shard, queries, 10)
    assert _same(got, R.topk(emb.cpu().numpy(), ids.cpu().numpy(), queries.cpu().numpy(), 10))
    emb16, _ = retrieval.embed_resident(Fake(), loader(), torch.device("cuda"))
    assert emb16.dtype == torch.float16 and torch.equal(emb16, emb.half())
    empty, _ = retrieval.embed_resident(Fake(), [], torch.device("cuda"), dtype=torch.float32)
    assert empty.dtype == torch.float32 and empty.shape[0] == 0


def test_query_and_pool_dtypes():
    from uniir_amd import retrieval
    pool, ids, q, _ = _f32_case(1000, 7, 64, 10)
    shard = _shard(pool, ids)
    q16 = torch.from_numpy(q).to(DEV).half()
    s, i = retrieval.search_shard(shard, q16, 10)
    ws, wi = retrieval.search_shard(shard, q16.float(), 10)
    assert torch.equal(i, wi) and torch.equal(s, ws)
    with pytest.raises(RuntimeError):
        retrieval.PoolShard(torch.from_numpy(pool).to(DEV).bfloat16(), torch.from_numpy(ids).to(DEV))
    with pytest.raises(RuntimeError):
        retrieval.PoolShard(torch.from_numpy(pool), torch.from_numpy(ids))                   # a CPU tensor
    with pytest.raises(RuntimeError):
        retrieval.PoolShard(torch.zeros(8, 100, device=DEV), torch.arange(8, device=DEV))    # dim % 64
