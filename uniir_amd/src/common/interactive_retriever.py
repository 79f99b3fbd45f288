"""Embeds ad-hoc queries and retrieves their candidates (drop-in for UniIR src/common/interactive_retriever.py).

Modality, InteractiveRetriever(cand_index_path, candidates_path, dataset_name, config), add_queries (:72-99) and
retrieve(k, batch_size) (:175-201) keep their names, checks, qid / task-id assignment and results.  The towers take their
fp16 forward through mbeir_embedder (the reference: autocast, :150-155) and the exact top-k is mbeir_retriever's device
search over the same cached pool shards as search_index.  Not copied, result-preserving:
  * the query embeddings stay in HBM (the reference round-trips them through ./interactive_queries_embed.npy, :158-171);
  * the model is built once per process and config (the reference rebuilds it per instance, i.e. per UniRAG dataset) and
    is not wrapped in DDP (inference only: every rank holds the full weights and embeds its contiguous slice);
  * a candidate jsonl is parsed once per (path, mtime) and shared with mbeir_retriever.get_raw_retrieved_candidates (the
    reference parses the union pool twice per dataset, :58-64 and mbeir_retriever.py:249-254).
"""
import os as _os
import sys as _sys

_SRC = _os.path.dirname(_os.path.dirname(_os.path.abspath(__file__)))          # <repo>/uniir_amd/src
for _p in (_os.path.dirname(_os.path.dirname(_SRC)), _SRC, _os.path.join(_SRC, "common")):
    if _p not in _sys.path:
        _sys.path.insert(0, _p)

import json
import os
from enum import Enum

from config import OmegaConf
from data.preprocessing.utils import DATASET_IDS, MBEIR_TASK, unhash_did

_CAND_CACHE = {}
_MODEL_CACHE = {}


class Modality(Enum):
    TEXT = "text"
    IMAGE = "image"
    IMAGE_TEXT = "image,text"


def load_candidates_by_did(candidates_path):
    """{did: record} of a candidate jsonl, in file order; cached per (path, mtime), one file at a time (the union pool is
    5.6 M records)"""
    key = (candidates_path, os.path.getmtime(candidates_path))
    if key not in _CAND_CACHE:
        _CAND_CACHE.clear()
        did_to_candidates = {}
        with open(candidates_path, "r") as f:
            for line in f:
                c = json.loads(line.strip())
                assert c["did"] not in did_to_candidates, "dids must be unique"
                did_to_candidates[c["did"]] = c
        _CAND_CACHE[key] = did_to_candidates
    return _CAND_CACHE[key]


def _query_embedder(config):
    """(model, img_preprocess_fn, tokenizer) for this config, built on its dist_config.gpu_id once per process"""
    from utils import build_model_from_config
    key = OmegaConf.to_yaml(config, sort_keys=True)
    if key not in _MODEL_CACHE:
        _MODEL_CACHE.clear()
        model = build_model_from_config(config)
        model.eval()
        if not callable(getattr(model, "encode_mbeir_batch")):
            raise AttributeError("The provided model does not have a callable 'encode' method.")
        if not callable(getattr(model, "get_img_preprocess_fn")):
            raise AttributeError("The provided model does not have an 'img_preprocess_fn' attribute.")
        if not callable(getattr(model, "get_tokenizer")):
            raise AttributeError("The provided model does not have a 'tokenizer' attribute.")
        img_preprocess_fn, tokenizer = model.get_img_preprocess_fn(), model.get_tokenizer()
        model = model.to(config.dist_config.gpu_id)
        print(f"Model is set up on GPU {config.dist_config.gpu_id}.")
        _MODEL_CACHE[key] = (model, img_preprocess_fn, tokenizer)
    return _MODEL_CACHE[key]


class InteractiveRetriever:
    def __init__(self, cand_index_path: str, candidates_path: str, dataset_name, config):
        import dist_utils
        from utils import set_seed
        set_seed(config.seed + dist_utils.get_rank())      # instruction prompts are a random choice: the seed is part of the result
        self.dataset_id = DATASET_IDS[dataset_name]
        self.model, self.img_preprocess_fn, self.tokenizer = _query_embedder(config)
        self.cand_index_path = cand_index_path
        self.config = config
        self.queries = []
        self.did_to_candidates = load_candidates_by_did(candidates_path)

    def add_queries(self, queries):
        """queries: (query_modality, query_txt, query_img_path, candidate_modality) tuples"""
        for query_modality, query_txt, query_img_path, candidate_modality in queries:
            if query_modality == Modality.TEXT.value:
                assert query_txt, "Query with 'text' modality must have non-null 'query_txt'"
                assert query_img_path is None, "Query with 'text' modality must have null 'query_img_path'"
            elif query_modality == Modality.IMAGE.value:
                assert query_txt is None, "Query with 'image' modality must have null 'query_txt'"
                assert query_img_path, "Query with 'image' modality must have non-null 'query_img_path'"
            elif query_modality == Modality.IMAGE_TEXT.value:
                assert query_txt, "Query with 'image' modality must have non-null 'query_txt'"
                assert query_img_path, "Query with 'image' modality must have non-null 'query_img_path'"
            else:
                raise ValueError("Only 'text', 'image' and 'image,text' query modalities are supported.")
            task_id = MBEIR_TASK[" -> ".join([query_modality, candidate_modality])]
            self.queries.append({
                "qid": ":".join([str(self.dataset_id), str(len(self.queries) + 1)]),    # dataset_id:query_num, counted across calls
                "query_modality": query_modality,
                "query_txt": query_txt,
                "query_img_path": query_img_path,
                "task_id": task_id,
                "candidate_modality": candidate_modality,
            })

    def _embed_queries(self):
        """-> fp16 [len(self.queries), d] on this rank's device, in add order (every rank holds all of them)"""
        import dist_utils
        from torch.utils.data import DataLoader
        from data.mbeir_dataset import MBEIRInferenceOnlyCollator, MBEIRInferenceOnlyDataset
        from mbeir_embedder import generate_embeds_and_ids_on_device
        data_config = self.config.data_config
        image_size = tuple(map(int, str(data_config.image_size).split(",")))
        main = dist_utils.is_main_process()
        if main:
            print(f"\nEmbedder Log: Generating embeddings for {len(self.queries)} queries.")
        dataset = MBEIRInferenceOnlyDataset(self.config.mbeir_data_dir, self.queries, data_config.query_instruct_path,
                                            self.img_preprocess_fn, enable_query_instruct=data_config.enable_query_instruct,
                                            print_config=main)
        collator = MBEIRInferenceOnlyCollator(tokenizer=self.tokenizer, image_size=image_size)
        sampler = dist_utils.ContiguousDistributedSampler(dataset, num_replicas=dist_utils.get_world_size(),
                                                          rank=dist_utils.get_rank())
        loader = DataLoader(dataset, batch_size=self.config.dataloader_config.batch_size,
                            num_workers=self.config.dataloader_config.num_workers, pin_memory=True, sampler=sampler,
                            shuffle=False, collate_fn=collator, drop_last=False)
        if main:
            print(f"Inference with half precision: {self.config.embed_config.use_fp16}")
        emb, _ = generate_embeds_and_ids_on_device(self.model, loader, self.config.dist_config.gpu_id,
                                                   use_fp16=self.config.embed_config.use_fp16)
        return emb

    def retrieve(self, k: int = 1, batch_size: int = 100):
        """the top-k candidate records of every added query, in add order"""
        from mbeir_retriever import search_embeddings
        if not self.queries:
            return []
        emb = self._embed_queries()
        print(f"Retriever: Searching with k={k}")
        _, retrieved_indices = search_embeddings(emb, self.cand_index_path, batch_size=batch_size, num_cand_to_retrieve=k)
        return [[self.did_to_candidates[unhash_did(int(h))] for h in indices] for indices in retrieved_indices]
