"""UNIIR_POOL_FP32 end to end on the tiny CLIP_SF model and two-batch loader of test_embed_fp32_pipeline_gpu.py: with the switch, the
fp32 embedding forward and use_fp16: False the embedder returns the fp32 rows of the forward, create_index keeps them, search_index
searches them (tests/topk_f32_ref.py bit for bit); without the switch, or under use_fp16: True, every array is fp16 as before."""
import os
import types

import numpy as np
import pytest
import torch

import topk_f32_ref as R
from test_embed_fp32_pipeline_gpu import _clip_sf, _embedder

pytestmark = pytest.mark.gpu


def _retriever():
    _embedder()                      # puts uniir_amd/src and uniir_amd/src/common on sys.path
    import mbeir_retriever
    return mbeir_retriever


def _index_config(root, dim):
    return types.SimpleNamespace(
        uniir_dir=str(root), experiment=types.SimpleNamespace(path_suffix="tiny"),
        index_config=types.SimpleNamespace(embed_dir_name="embed", index_dir_name="index", faiss_config=types.SimpleNamespace(dim=dim),
                                           cand_pools_config=types.SimpleNamespace(enable_idx=True, cand_pools_name_to_idx=["toy"])))


def test_fp32_rows_from_the_embedder_to_the_search(monkeypatch, tmp_path):
    from oracle import c_oracle
    E, M = _embedder(), _retriever()
    model, switch, loader = _clip_sf()
    switch.embed_fp32 = True

    def extract(use_fp16=False):
        emb, ids = E.generate_embeds_and_ids_for_dataset_with_gather(model, loader(), "cuda:0", use_fp16=use_fp16)
        assert ids == list(range(4)) and emb.shape == (4, 64)
        return emb

    monkeypatch.delenv("UNIIR_POOL_FP32", raising=False)
    off = extract()
    assert off.dtype == np.float16
    monkeypatch.setenv("UNIIR_POOL_FP32", "1")
    on = extract()
    assert on.dtype == np.float32 and switch.precision == "bf16"
    # the fp32 forward by hand, batch by batch
    switch.precision = "fp32"
    with torch.no_grad():
        rows = []
        for batch in loader():
            batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
            rows.append(model(batch, encode_mbeir_batch=True)[0])
    switch.precision = "bf16"
    by_hand = torch.cat(rows)
    assert by_hand.dtype == torch.float32 and np.array_equal(on, by_hand.cpu().numpy())
    assert np.array_equal(on.astype(np.float16), off) and not np.array_equal(on, off.astype(np.float32))
    half = extract(use_fp16=True)                     # use_fp16: True ignores the switch
    assert half.dtype == np.float16
    monkeypatch.delenv("UNIIR_POOL_FP32")
    assert np.array_equal(extract(use_fp16=True), half) and np.array_equal(extract(), off)

    # a larger pool around the model's rows, written as the embedder writes it
    rng = np.random.default_rng(5)
    pool = np.concatenate([on, (rng.standard_normal((996, 64)) * 0.05).astype(np.float32)])
    ids = (rng.permutation(1000).astype(np.int64) * 7 + 3)
    embed_dir = tmp_path / "embed" / "tiny" / "cand_pool"
    os.makedirs(embed_dir)
    np.save(embed_dir / "mbeir_toy_cand_pool_embed.npy", pool)
    np.save(embed_dir / "mbeir_toy_cand_pool_ids.npy", ids)
    q32, q16 = str(tmp_path / "q32.npy"), str(tmp_path / "q16.npy")
    queries = np.concatenate([on, rng.standard_normal((5, 64)).astype(np.float32)])
    np.save(q32, queries)
    np.save(q16, queries.astype(np.float16))
    index_path = str(tmp_path / "index" / "tiny" / "cand_pool" / "mbeir_toy_cand_pool.index")
    cfg = _index_config(tmp_path, 64)

    def stored():
        with np.load(index_path) as z:
            return z["emb"], z["ids"]

    try:
        # without the switch: the fp16 container and the fp16 search of before, whatever the .npy holds
        M._SHARD_CACHE.clear()
        M.create_index(cfg)
        emb16, sid = stored()
        assert emb16.dtype == np.float16 and np.array_equal(emb16, pool.astype(np.float16)) and np.array_equal(sid, ids)
        s, i = M.search_index(q32, index_path, batch_size=4, num_cand_to_retrieve=10)
        ws, wi = c_oracle.topk(emb16, ids, queries.astype(np.float16), 10)
        assert np.array_equal(i, wi) and np.array_equal(s, ws)
        # with it: fp32 rows kept and searched; fp32 queries as they are, fp16 queries cast up
        monkeypatch.setenv("UNIIR_POOL_FP32", "1")
        M._SHARD_CACHE.clear()
        M.create_index(cfg)
        emb32, sid = stored()
        assert emb32.dtype == np.float32 and np.array_equal(emb32, pool) and np.array_equal(sid, ids)
        assert M._device_shards(index_path)[0].emb.dtype == torch.float32
        s, i = M.search_index(q32, index_path, batch_size=4, num_cand_to_retrieve=10)
        ws, wi = R.topk(emb32, ids, queries, 10)
        assert np.array_equal(i, wi) and np.array_equal(s, ws)
        s, i = M.search_index(q16, index_path, batch_size=16, num_cand_to_retrieve=10)
        ws, wi = R.topk(emb32, ids, queries.astype(np.float16).astype(np.float32), 10)
        assert np.array_equal(i, wi) and np.array_equal(s, ws)
    finally:
        M._SHARD_CACHE.clear()
