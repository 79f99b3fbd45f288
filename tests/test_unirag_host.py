"""UniRAG host logic against the reference-generated golden (tests/golden/g16_unirag.json, make_golden_unirag.py):
get_raw_retrieved_candidates with a stub complement retriever, the written jsonl bytes, InteractiveRetriever.add_queries
(qids / task ids over two calls, the errors of invalid tuples).  CPU only."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "uniir_amd", "src")
for p in (ROOT, SRC, os.path.join(SRC, "common")):
    if p not in sys.path:
        sys.path.insert(0, p)

G = json.load(open(os.path.join(ROOT, "tests", "golden", "g16_unirag.json")))


class StubComplementRetriever:
    """the golden's stub: the n-th complement query gets the records of complement_topk[n % len]"""

    def __init__(self, did_to_cand):
        self.did_to_cand, self.queries, self.k = did_to_cand, [], None

    def add_queries(self, queries):
        self.queries.extend(list(q) for q in queries)

    def retrieve(self, k=1, batch_size=100):
        self.k = k
        top = G["complement_topk"]
        return [[self.did_to_cand[d] for d in top[n % len(top)]] for n in range(len(self.queries))]


@pytest.fixture()
def files(tmp_path):
    q, c = tmp_path / "q.jsonl", tmp_path / "c.jsonl"
    q.write_text("".join(json.dumps(r) + "\n" for r in G["queries"]))
    c.write_text("".join(json.dumps(r) + "\n" for r in G["candidates"]))
    return str(q), str(c)


def test_raw_candidates_without_complements_equal_the_reference(files):
    import mbeir_retriever
    got = mbeir_retriever.get_raw_retrieved_candidates(files[0], files[1], G["retrieved_indices"], G["hashed_qids"], None)
    assert [[k, v] for k, v in got.items()] == G["raw_plain"]


def test_raw_candidates_with_complements_equal_the_reference(files):
    import mbeir_retriever
    stub = StubComplementRetriever({c["did"]: c for c in G["candidates"]})
    got = mbeir_retriever.get_raw_retrieved_candidates(files[0], files[1], G["retrieved_indices"], G["hashed_qids"], stub)
    assert [[k, v] for k, v in got.items()] == G["raw_complement"]
    assert stub.queries == G["complement_queries"] and stub.k == G["complement_k"] == 10
    comps = [c for _, v in G["raw_complement"] for c in v["complement_candidates"]]
    assert None in comps                                   # the case with no qualifying result is covered


def test_written_jsonl_is_json_dump_of_the_golden(files, tmp_path):
    import mbeir_retriever
    stub = StubComplementRetriever({c["did"]: c for c in G["candidates"]})
    got = mbeir_retriever.get_raw_retrieved_candidates(files[0], files[1], G["retrieved_indices"], G["hashed_qids"], stub)
    out = tmp_path / "r_retrieved.jsonl"
    mbeir_retriever.write_retrieved_jsonl(got, str(out))
    want = "".join(json.dumps(v) + "\n" for _, v in G["raw_complement"])
    assert out.read_bytes() == want.encode()


def test_candidate_jsonl_is_parsed_once_per_path_and_mtime(files):
    import interactive_retriever as ir
    a = ir.load_candidates_by_did(files[1])
    assert ir.load_candidates_by_did(files[1]) is a
    assert list(a) == [c["did"] for c in G["candidates"]]
    os.utime(files[1], (1, 1))                             # a rewritten file is read again
    assert ir.load_candidates_by_did(files[1]) is not a


def _fresh():
    import interactive_retriever as ir
    from data.preprocessing.utils import DATASET_IDS
    r = object.__new__(ir.InteractiveRetriever)
    r.dataset_id, r.queries = DATASET_IDS["MSCOCO"], []
    return r


def test_add_queries_qids_and_task_ids_equal_the_reference():
    r = _fresh()
    calls = [[["text", "a cat", None, "image"], ["image", None, "img/x.jpg", "text"], ["text", "a bus", None, "image,text"]],
             [["image,text", "t", "img/y.jpg", "image,text"], ["image", None, "img/z.jpg", "image"], ["text", "q", None, "text"]]]
    for call, want in zip(calls, G["add"]):
        r.add_queries([tuple(q) for q in call])
        assert r.queries == want


def test_add_queries_errors_equal_the_reference():
    for case in G["errors"]:
        r = _fresh()
        err = None
        try:
            r.add_queries([tuple(q) for q in case["call"]])
        except Exception as e:  # noqa: BLE001
            err = {"type": type(e).__name__, "msg": str(e)}
        assert err == case["error"], case["call"]
        assert r.queries == case["kept"]


def test_modality_enum():
    from interactive_retriever import Modality
    assert [m.value for m in Modality] == ["text", "image", "image,text"]
