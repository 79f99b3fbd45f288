"""CPU tests of the fp32 candidate-pool search: tests/topk_f32_ref.py (the numpy restatement of the contract) against the C oracle on
fp16-representable inputs, the sub-shard rule with 4-byte rows, and the host-side refusals of the new entry points (no device)."""
import ctypes
import inspect

import numpy as np
import pytest

import topk_f32_ref as R


def _case(n, nq, dim, seed):
    rng = np.random.default_rng(seed)
    pool = (rng.standard_normal((n, dim)) * 0.3).astype(np.float16)
    q = rng.standard_normal((nq, dim)).astype(np.float16)
    pool[n // 3] = 0                                     # a zero row (inverse norm 0)
    pool[n // 2] = pool[7]                               # duplicates: exact score ties, the id decides
    pool[n - 1] = pool[7]
    ids = rng.permutation(n).astype(np.int64) * 3 + 5
    return pool, ids, q


@pytest.mark.parametrize("n,nq,dim,k", [(5000, 7, 768, 10), (40030, 64, 768, 10), (3000, 5, 64, 50)])
def test_restatement_equals_the_c_oracle_bit_for_bit(n, nq, dim, k):
    from oracle import c_oracle
    pool, ids, q = _case(n, nq, dim, n + nq)
    ws, wi = c_oracle.topk(pool, ids, q, k)
    s, i = R.topk(pool.astype(np.float32), ids, q.astype(np.float32), k)
    assert np.array_equal(i, wi) and np.array_equal(s, ws)
    assert np.array_equal(R.inv_norms(pool.astype(np.float32)), c_oracle.inv_norms(pool))


def test_restatement_pads_missing_results():
    rng = np.random.default_rng(1)
    pool, q = rng.standard_normal((5, 64)).astype(np.float32), rng.standard_normal((3, 64)).astype(np.float32)
    s, i = R.topk(pool, np.arange(5) + 100, q, 10)
    assert np.all(i[:, 5:] == -1) and np.all(np.isneginf(s[:, 5:])) and np.all(i[:, :5] >= 100)
    assert np.all(np.diff(s[:, :5], axis=1) <= 0)


def test_subshard_bounds_with_four_byte_rows():
    from uniir_amd import retrieval
    assert list(inspect.signature(retrieval.subshard_bounds).parameters) == ["n", "dim", "itemsize"]
    assert retrieval.subshard_bounds(699_050, 768, 4) == [(0, 699_050)]                 # 699 050 * 3072 < 2 GiB
    for n in (700_000, 5_600_000):
        b = retrieval.subshard_bounds(n, 768, 4)
        assert len(b) > 1 and b[0][0] == 0 and b[-1][1] == n
        assert all(b[j][1] == b[j + 1][0] for j in range(len(b) - 1))
        per = b[0][1] - b[0][0]
        assert per % 32 == 0 and all(hi - lo == per for lo, hi in b[:-1]) and 0 < b[-1][1] - b[-1][0] <= per
        assert per * 768 * 4 < (1 << 31) and per <= retrieval.FUSED_TAIL_ROWS == 786_432
    # the two-byte default keeps the documented values: one range below 2 GiB, 8 ranges of 700 000 rows for the 5.6 M pool
    assert retrieval.subshard_bounds(1_398_101, 768) == [(0, 1_398_101)] == retrieval.subshard_bounds(1_398_101, 768, 2)
    b = retrieval.subshard_bounds(5_600_000, 768)
    assert len(b) == 8 and all(hi - lo == 700_000 for lo, hi in b)
    assert retrieval.subshard_bounds(1_398_102, 768) == [(0, 699_072), (699_072, 1_398_102)]


def test_fp32_entry_points_are_exported_and_refuse_on_the_host():
    """the new symbols exist, the workspace query is host arithmetic, and every shape / alignment refusal of uniir_topk_ip_f32 comes
    before the device is touched (these addresses are never dereferenced; this machine may have no GPU at all)"""
    from uniir_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("uniir_pool_inv_norms_f32", "uniir_topk_ip_f32_workspace_bytes", "uniir_topk_ip_f32"):
        assert name in _lib.SIGNATURES and hasattr(raw, name)
    ws = lib.uniir_topk_ip_f32_workspace_bytes
    assert ws(0, 10, 1000, 768) == 0 and ws(10, 0, 1000, 768) == 0
    need = ws(64, 10, 40_030, 768)
    assert need > 64 * 2502 * 4 + 2 * 64 * 36 * 16 * 4                     # group maxima + candidates + exact scores
    EINVAL, ESHAPE, EALIGN = -1, -2, -3
    A = 0x10000

    def call(rows=1000, dim=768, nq=4, k=10, pool=A, inv=A, q=A, w=A, wbytes=1 << 40):
        return lib.uniir_topk_ip_f32(pool, inv, A, rows, dim, q, nq, k, A, A, w, wbytes, None)

    assert call(dim=100) == ESHAPE
    assert call(k=57) == ESHAPE
    assert call(rows=700_000) == ESHAPE                                    # 700 000 * 768 * 4 >= 2 GiB
    assert call(pool=None) == EINVAL and call(nq=0) == EINVAL
    assert call(pool=A + 4) == EALIGN and call(w=A + 16) == EALIGN
    assert call(wbytes=16) == EINVAL                                       # workspace too small
    assert lib.uniir_pool_inv_norms_f32(None, 4, 64, A, None) == EINVAL
    assert lib.uniir_pool_inv_norms_f32(A, 4, 6, A, None) == ESHAPE
    assert lib.uniir_pool_inv_norms_f32(A + 4, 4, 64, A, None) == EALIGN
    assert lib.uniir_pool_inv_norms_f32(A, 0, 64, A, None) == 0


def test_create_index_keeps_fp32_rows_only_under_the_switch(monkeypatch, tmp_path):
    """host arithmetic only: the .index container holds the .npy's fp32 rows under UNIIR_POOL_FP32=1, fp16 otherwise (today's bytes);
    an fp16 .npy stays fp16 either way"""
    import os
    import sys
    import types
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (os.path.join(root, "uniir_amd", "src"), os.path.join(root, "uniir_amd", "src", "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import mbeir_retriever as M
    rng = np.random.default_rng(2)
    emb = rng.standard_normal((9, 64)).astype(np.float32)
    ids = np.arange(9, dtype=np.int64) + 70
    edir = tmp_path / "embed" / "x" / "cand_pool"
    os.makedirs(edir)
    np.save(edir / "mbeir_toy_cand_pool_ids.npy", ids)
    cfg = types.SimpleNamespace(
        uniir_dir=str(tmp_path), experiment=types.SimpleNamespace(path_suffix="x"),
        index_config=types.SimpleNamespace(embed_dir_name="embed", index_dir_name="index", faiss_config=types.SimpleNamespace(dim=64),
                                           cand_pools_config=types.SimpleNamespace(enable_idx=True, cand_pools_name_to_idx=["toy"])))
    path = tmp_path / "index" / "x" / "cand_pool" / "mbeir_toy_cand_pool.index"
    for env, stored, want in (("0", emb, np.float16), ("1", emb, np.float32), ("1", emb.astype(np.float16), np.float16),
                              (None, emb, np.float16)):
        if env is None:
            monkeypatch.delenv("UNIIR_POOL_FP32", raising=False)
        else:
            monkeypatch.setenv("UNIIR_POOL_FP32", env)
        np.save(edir / "mbeir_toy_cand_pool_embed.npy", stored)
        M.create_index(cfg)
        with np.load(path) as z:
            assert z["emb"].dtype == want and np.array_equal(z["emb"], stored.astype(want)) and np.array_equal(z["ids"], ids)


def test_pool_fp32_switch_is_read_when_used(monkeypatch):
    from uniir_amd import precision
    monkeypatch.delenv("UNIIR_POOL_FP32", raising=False)
    assert precision.pool_fp32() is False
    monkeypatch.setenv("UNIIR_POOL_FP32", "1")
    assert precision.pool_fp32() is True
    monkeypatch.setenv("UNIIR_POOL_FP32", "0")
    assert precision.pool_fp32() is False
