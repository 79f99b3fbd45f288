#!/usr/bin/env python
"""Generates tests/golden/g16_unirag.json by IMPORTING THE REFERENCE (read-only, the checkout make_golden.REF names): the
UniRAG host logic of src/common/mbeir_retriever.py and src/common/interactive_retriever.py.

Run:  python tests/golden/make_golden_unirag.py        (CPU only; needs the reference checkout)

Import shims: the stubs of make_golden.py (clip, torchvision.transforms, typeguard, faiss, omegaconf), plus tqdm where it
is not installed.  Recorded:
  raw         get_raw_retrieved_candidates on a hand-made query / candidate jsonl with a stub complement retriever that
              returns fixed top-10 lists: hits of all three modalities, complements whose first same-modality result is
              the query's own image or text (skipped), and one with no qualifying result (null)
  add         InteractiveRetriever.add_queries on an instance made without __init__: qids and task ids over two calls
  errors      the exceptions add_queries raises for invalid tuples (and how many queries were kept before the error)
"""
import importlib
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (sys.path: the reference's src and src/common first)

REF = make_golden.REF

# ------------------------------------------------------------------------------------------- the hand-made inputs
QUERIES = [
    {"qid": "9:1", "query_txt": "a dog on a red sofa", "query_img_path": None, "query_modality": "text",
     "query_src_content": None, "pos_cand_list": ["9:3"], "neg_cand_list": [], "task_id": 0},
    {"qid": "9:2", "query_txt": None, "query_img_path": "img/q2.jpg", "query_modality": "image",
     "query_src_content": None, "pos_cand_list": ["9:4"], "neg_cand_list": [], "task_id": 3},
    {"qid": "9:3", "query_txt": "what colour is this éclair", "query_img_path": "img/q3.jpg",
     "query_modality": "image,text", "query_src_content": None, "pos_cand_list": ["9:7"], "neg_cand_list": [],
     "task_id": 6},
]
CANDS = [
    {"txt": None, "img_path": "img/c1.jpg", "modality": "image", "did": "9:1", "src_content": None},
    {"txt": "a dog on a red sofa", "img_path": None, "modality": "text", "did": "9:2", "src_content": None},   # = query 9:1's text
    {"txt": None, "img_path": "img/c3.jpg", "modality": "image", "did": "9:3", "src_content": None},
    {"txt": "a cat asleep", "img_path": None, "modality": "text", "did": "9:4", "src_content": None},
    {"txt": None, "img_path": "img/q2.jpg", "modality": "image", "did": "9:5", "src_content": None},           # = query 9:2's image
    {"txt": "two birds", "img_path": "img/c6.jpg", "modality": "image,text", "did": "9:6", "src_content": None},
    {"txt": "a chocolate éclair", "img_path": "img/c7.jpg", "modality": "image,text", "did": "9:7", "src_content": None},
    {"txt": "a red bus \"quoted\"", "img_path": None, "modality": "text", "did": "9:8", "src_content": None},
    {"txt": None, "img_path": "img/q3.jpg", "modality": "image", "did": "9:9", "src_content": None},           # = query 9:3's image
    {"txt": "what colour is this éclair", "img_path": None, "modality": "text", "did": "9:10", "src_content": None},
    {"txt": None, "img_path": "img/c11.jpg", "modality": "image", "did": "1:11", "src_content": "{\"k\": 1}"},
    {"txt": "", "img_path": None, "modality": "text", "did": "1:12", "src_content": None},                     # empty text
]
RETRIEVED = {              # top-4 dids per query, in query order: all three modalities among the hits
    "9:1": ["9:2", "9:1", "9:6", "9:4"],
    "9:2": ["9:5", "9:4", "9:7", "1:11"],
    "9:3": ["9:7", "9:10", "9:9", "9:8"],
}
# the stub complement retriever's top-10 for the n-th complement query (cycled): a same-modality hit equal to the original
# query first, non-matching modalities, an empty text, and one list with no qualifying entry at all
COMPLEMENT_TOPK = [
    ["9:6", "9:2", "9:1", "9:3", "9:4", "9:5", "9:7", "9:8", "9:9", "9:10"],
    ["9:7", "1:12", "9:2", "9:10", "9:8", "9:4", "9:1", "9:3", "9:5", "9:6"],
    ["9:6", "9:7", "9:9", "9:5", "9:3", "1:11", "9:1", "9:2", "9:4", "9:8"],
    ["9:6", "9:7", "9:6", "9:7", "9:6", "9:7", "9:6", "9:7", "9:6", "9:7"],
    ["9:5", "9:9", "9:1", "9:2", "9:3", "9:4", "9:6", "9:7", "9:8", "9:10"],
    ["9:2", "9:10", "9:8", "9:1", "9:3", "9:4", "9:5", "9:6", "9:7", "9:9"],
    ["1:12", "9:2", "9:4", "9:1", "9:3", "9:5", "9:6", "9:7", "9:8", "9:9"],
]

ADD_CALLS = [
    [["text", "a cat", None, "image"], ["image", None, "img/x.jpg", "text"], ["text", "a bus", None, "image,text"]],
    [["image,text", "t", "img/y.jpg", "image,text"], ["image", None, "img/z.jpg", "image"], ["text", "q", None, "text"]],
]
BAD_CALLS = [
    [["text", "t", "img/a.jpg", "image"]],
    [["text", "", None, "image"]],
    [["text", None, None, "image"]],
    [["image", "t", "img/a.jpg", "text"]],
    [["image", None, None, "text"]],
    [["image,text", None, "img/a.jpg", "text"]],
    [["image,text", "t", None, "text"]],
    [["audio", "t", None, "text"]],
    [["text", "t", None, "audio"]],
    [["text", "ok", None, "image"], ["image,text", "t", "", "text"]],
]


class StubComplementRetriever:
    """records the complement queries; retrieve(k) answers the n-th with the candidate records of COMPLEMENT_TOPK[n % 7]"""

    def __init__(self, did_to_cand):
        self.did_to_cand, self.queries, self.k = did_to_cand, [], None

    def add_queries(self, queries):
        self.queries.extend(list(q) for q in queries)

    def retrieve(self, k=1, batch_size=100):
        self.k = k
        return [[self.did_to_cand[d] for d in COMPLEMENT_TOPK[n % len(COMPLEMENT_TOPK)]] for n in range(len(self.queries))]


def _write_jsonl(path, rows):
    with open(path, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


def main():
    import tempfile
    import transformers  # noqa: F401  (the reference embedder imports it; it must not see the torchvision stub)
    make_golden._install_stubs()
    try:
        import tqdm  # noqa: F401
    except ImportError:
        sys.modules["tqdm"] = types.ModuleType("tqdm")
    ir = importlib.import_module("interactive_retriever")
    mr = importlib.import_module("mbeir_retriever")
    assert ir.__file__.startswith(REF) and mr.__file__.startswith(REF), (ir.__file__, mr.__file__)
    from data.preprocessing.utils import DATASET_IDS, hash_did, hash_qid
    out = {"queries": QUERIES, "candidates": CANDS, "complement_topk": COMPLEMENT_TOPK}
    with tempfile.TemporaryDirectory() as tmp:
        qpath, cpath = os.path.join(tmp, "q.jsonl"), os.path.join(tmp, "c.jsonl")
        _write_jsonl(qpath, QUERIES)
        _write_jsonl(cpath, CANDS)
        hashed_qids = [hash_qid(q["qid"]) for q in QUERIES]
        retrieved = [[hash_did(d) for d in RETRIEVED[q["qid"]]] for q in QUERIES]
        out["hashed_qids"], out["retrieved_indices"] = hashed_qids, retrieved
        plain = mr.get_raw_retrieved_candidates(qpath, cpath, retrieved, hashed_qids, None)
        stub = StubComplementRetriever({c["did"]: c for c in CANDS})
        full = mr.get_raw_retrieved_candidates(qpath, cpath, retrieved, hashed_qids, stub)
    out["raw_plain"] = list(plain.items())
    out["raw_complement"] = list(full.items())
    out["complement_queries"], out["complement_k"] = stub.queries, stub.k
    nulls = sum(c is None for v in full.values() for c in v["complement_candidates"])
    assert nulls >= 1 and len(stub.queries) >= 6, (nulls, len(stub.queries))

    def fresh():
        r = object.__new__(ir.InteractiveRetriever)
        r.dataset_id, r.queries = DATASET_IDS["MSCOCO"], []
        return r

    r = fresh()
    out["add"] = []
    for call in ADD_CALLS:
        r.add_queries([tuple(q) for q in call])
        out["add"].append([dict(q) for q in r.queries])
    out["errors"] = []
    for call in BAD_CALLS:
        r = fresh()
        try:
            r.add_queries([tuple(q) for q in call])
            err = None
        except Exception as e:  # noqa: BLE001
            err = {"type": type(e).__name__, "msg": str(e)}
        out["errors"].append({"call": call, "error": err, "kept": [dict(q) for q in r.queries]})
    with open(os.path.join(HERE, "g16_unirag.json"), "w") as f:
        json.dump(out, f, indent=1)
    print("g16 ok", len(stub.queries), "complement queries,", nulls, "null")


if __name__ == "__main__":
    main()
