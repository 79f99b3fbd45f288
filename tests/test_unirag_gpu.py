"""UniRAG evaluation on a tiny synthetic M-BEIR tree: embed -> index -> run_retrieval with raw_retrieval and
retrieve_image_text_pairs on (reference README "UniRAG evaluation", configs_scripts/large/eval/unirag).  Random-init
towers and ONE instruction prompt per (dataset, query modality, candidate modality) row, so embeddings are deterministic.
Checked: run files and recalls equal the raw_retrieval: false run; "candidates" are the pool records of the run file's
ids; "complement_candidates" equal a restatement (complement queries embedded independently, the C oracle's exact top-10,
the selection rule); a standalone InteractiveRetriever returns the C oracle's top-k; BLIP_FF (small) passes the same;
two ranks on one GPU write the same bytes as one."""
import json
import os
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "uniir_amd", "src")
for p in (ROOT, SRC, os.path.join(SRC, "common")):
    if p not in sys.path:
        sys.path.insert(0, p)

MODS = ("text", "image", "image,text")
N_CAND, N_QUERY = 30, 8


def _toy_clip_tokenize(texts, context_length=77, truncate=True):
    out = torch.zeros(len(texts), context_length, dtype=torch.int32)
    for i, t in enumerate(texts):
        ids = [510] + [1 + (sum(map(ord, w)) % 500) for w in t.split()][: context_length - 2] + [511]
        out[i, : len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return out


def _toy_bert_tokenize(texts, max_len=20):
    from transformers import BatchEncoding
    ids = torch.zeros(len(texts), max_len, dtype=torch.long)
    mask = torch.zeros(len(texts), max_len, dtype=torch.long)
    for i, t in enumerate(texts):
        row = [1] + [4 + (sum(map(ord, w)) % 190) for w in t.split()][: max_len - 2] + [2]
        ids[i, : len(row)], mask[i, : len(row)] = torch.tensor(row), 1
    return BatchEncoding({"input_ids": ids, "attention_mask": mask})


def _make_tree(root):
    from PIL import Image
    rng = np.random.default_rng(1)
    for sub in ("img", "val", "cand_pool", "instructions", "qrels/val"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    words = ["red", "blue", "dog", "cat", "tree", "car", "river", "house", "bird", "stone", "cloud", "road"]
    cands = []
    for i in range(N_CAND):
        mod = MODS[(i + 2) % 3]
        rec = {"txt": " ".join(rng.choice(words, 4)) if "text" in mod else None, "img_path": None, "modality": mod,
               "did": f"9:{i + 1}", "src_content": None}
        if "image" in mod:
            rec["img_path"] = f"img/c{i}.png"
            Image.fromarray(rng.integers(0, 255, (40, 52, 3), dtype=np.uint8)).save(os.path.join(root, rec["img_path"]))
        cands.append(rec)
    for name in ("mbeir_toy_cand_pool.jsonl", "mbeir_toy_val_cand_pool.jsonl"):    # embedder's / UniRAG's file name
        with open(os.path.join(root, "cand_pool", name), "w") as f:
            f.writelines(json.dumps(c) + "\n" for c in cands)
    queries, qrels = [], []
    for i in range(N_QUERY):
        pos = cands[(3 * i) % N_CAND]
        qm = MODS[i % 3]          # text, image and image+text queries: hits of every modality for either model
        q = {"qid": f"9:{i + 1}", "query_txt": " ".join(rng.choice(words, 3)) if "text" in qm else None,
             "query_img_path": cands[(3 * i + 3) % N_CAND]["img_path"] if "image" in qm else None,   # the pool's own images
             "query_modality": qm, "query_src_content": None, "pos_cand_list": [pos["did"]], "neg_cand_list": [],
             "task_id": {"image": 0, "text": 1, "image,text": 2}[pos["modality"]]}
        if i == 2:                # the query's own text sits in the pool as well: a complement must skip it
            q["query_txt"] = cands[1]["txt"]
        queries.append(q)
        qrels.append(f"{q['qid']} 0 {pos['did']} 1 {q['task_id']}")
    with open(os.path.join(root, "val", "mbeir_toy_val.jsonl"), "w") as f:
        f.writelines(json.dumps(q) + "\n" for q in queries)
    with open(os.path.join(root, "qrels", "val", "mbeir_toy_val_qrels.txt"), "w") as f:
        f.write("\n".join(qrels) + "\n")
    with open(os.path.join(root, "instructions", "query_instructions.tsv"), "w") as f:
        f.write("query_modality\tcand_modality\tdataset_name\tdataset_id\tprompt_1\n")
        for qm in MODS:
            for cm in MODS:
                f.write(f"{qm}\t{cm}\tToy\t9\tfind the {cm.replace(',', ' and ')} for this {qm.replace(',', ' and ')}\n")
    return cands, queries


def _configs(tmp, kind):
    model = {"clip": """
model:
  name: "CLIPScoreFusion"
  short_name: "CLIP_SF"
  clip_vision_model_name: "tiny-test"
  pretrained_clip_model_dir: "checkpoint/CLIP/"
  ckpt_config: {ckpt_dir: "checkpoint/toy/", ckpt_name: "clip_sf.pth"}
""", "blip": """
model:
  name: "BLIPFeatureFusion"
  short_name: "BLIP_FF"
  ckpt_config: {ckpt_dir: "checkpoint/toy/", ckpt_name: "blip_ff.pth"}
"""}[kind]
    size = "64, 64" if kind == "clip" else "32, 32"
    common = model + """
experiment: {instruct_status: "Instruct", path_suffix: "${model.short_name}/${experiment.instruct_status}/"}
seed: 2023
dist_config: {dist_url: "env://"}
"""
    embed = common + f"""
embed_config:
  embed_dir_name: "embed"
  use_fp16: True
  val_datasets_config: {{enable_embed: True, datasets_name: ["toy"], correspond_cand_pools_name: ["toy"]}}
  cand_pools_config: {{enable_embed: True, embed_union_pool: False, cand_pools_name_to_embed: ["toy"]}}
dataloader_config: {{num_workers: 0, batch_size: 5}}
data_config:
  image_size: {size}
  shuffle_cand: False
  enable_query_instruct: True
  train_dir_name: "train"
  val_dir_name: "val"
  test_dir_name: "test"
  cand_pool_dir_name: "cand_pool"
  query_instruct_path: instructions/query_instructions.tsv
"""
    dim = 64 if kind == "clip" else 128
    index = common + f"""
index_config:
  faiss_config: {{idx_type: Flat, dim: {dim}, metric: METRIC_INNER_PRODUCT}}
  embed_dir_name: "embed"
  index_dir_name: "index"
  cand_pools_config: {{enable_idx: True, cand_pools_name_to_idx: ["toy"]}}
"""
    retrieval = common + """
retrieval_config:
  embed_dir_name: "embed"
  index_dir_name: "index"
  results_dir_name: "retrieval_results"
  qrel_dir_name: "qrels"
  query_dir_name: ""
  candidate_dir_name: "cand_pool"
  write_to_tsv: True
  raw_retrieval: False
  retrieve_image_text_pairs: True
  val_datasets_config:
    enable_retrieve: True
    datasets_name: ["toy"]
    correspond_cand_pools_name: ["toy"]
    correspond_qrels_name: ["toy"]
    correspond_metrics_name: ["Recall@1, Recall@5, Recall@10"]
"""
    paths = {}
    for name, txt in dict(embed=embed, index=index, retrieval=retrieval).items():
        paths[name] = os.path.join(tmp, f"{kind}_{name}.yaml")
        with open(paths[name], "w") as f:
            f.write(txt)
    return paths


def _load(path, uniir_dir, data_dir, distributed=False):
    from config import OmegaConf
    c = OmegaConf.load(path)
    c.uniir_dir, c.mbeir_data_dir = uniir_dir, data_dir
    c.dist_config.gpu_id, c.dist_config.distributed_mode = 0, distributed
    return c


def _blip_model(state_path=None):
    from models.uniir_blip.blip_featurefusion.blip_ff import BLIPFeatureFusion
    import types
    z = np.load(os.path.join(ROOT, "tests", "golden", "g8_blipff.npz"))
    med, vit = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    m = BLIPFeatureFusion(med_config=med, vit_config=vit, embed_dim=med["hidden_size"], queue_size=16,
                          config=types.SimpleNamespace(tokenizer_max_length=20))
    if state_path:
        m.load_state_dict(torch.load(state_path, map_location="cpu")["model"])
    m.get_tokenizer = lambda: _toy_bert_tokenize          # offline stand-in for the bert-base-uncased vocabulary
    return m


def _patch_models(kind, uniir_dir, setattr_=setattr):
    """CLIP: the tiny config and the toy tokenizer.  BLIP: build_model_from_config builds the small BLIP_FF from the saved
    weights (the factory builds the base / large ViT of the configs)."""
    from oracle import clip_oracle as O
    from uniir_amd import clip_front, clip_model
    import mbeir_embedder
    clip_model.CLIP_CONFIGS["tiny-test"] = O.tiny_config()
    setattr_(clip_front, "tokenize", _toy_clip_tokenize)
    if kind == "blip":
        utils_mod = sys.modules[mbeir_embedder.build_model_from_config.__module__]
        factory = lambda config: _blip_model(os.path.join(uniir_dir, "checkpoint/toy/blip_ff.pth"))   # noqa: E731
        setattr_(mbeir_embedder, "build_model_from_config", factory)
        setattr_(utils_mod, "build_model_from_config", factory)


def _prepare(tmp_path, kind, monkeypatch):
    """tree + weights + embed + index; -> (data_dir, uniir_dir, config paths, candidates, queries)"""
    from oracle import clip_oracle as O
    data_dir, uniir_dir = str(tmp_path / "mbeir"), str(tmp_path / "uniir")
    cands, queries = _make_tree(data_dir)
    cfgs = _configs(str(tmp_path), kind)
    os.makedirs(os.path.join(uniir_dir, "checkpoint/CLIP"), exist_ok=True)
    os.makedirs(os.path.join(uniir_dir, "checkpoint/toy"), exist_ok=True)
    _patch_models(kind, uniir_dir, monkeypatch.setattr)
    if kind == "clip":
        from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
        torch.save({"state_dict": O.init_state_dict(O.tiny_config(), seed=4)},
                   os.path.join(uniir_dir, "checkpoint/CLIP/tiny-test.pt"))
        m = CLIPScoreFusion(model_name="tiny-test", download_root=os.path.join(uniir_dir, "checkpoint/CLIP"))
        torch.save({"model": m.state_dict()}, os.path.join(uniir_dir, "checkpoint/toy/clip_sf.pth"))
    else:
        torch.manual_seed(11)
        torch.save({"model": _blip_model().state_dict()}, os.path.join(uniir_dir, "checkpoint/toy/blip_ff.pth"))
    import mbeir_embedder
    import mbeir_retriever
    mbeir_embedder.main(_load(cfgs["embed"], uniir_dir, data_dir))
    mbeir_retriever.create_index(_load(cfgs["index"], uniir_dir, data_dir))
    return data_dir, uniir_dir, cfgs, cands, queries


def _embed_independently(cfg, queries):
    """the queries through a freshly built model, the inference-only dataset / collator and the fp16 extraction"""
    import mbeir_embedder
    from torch.utils.data import DataLoader
    from data.mbeir_dataset import MBEIRInferenceOnlyCollator, MBEIRInferenceOnlyDataset
    model = mbeir_embedder.build_model_from_config(cfg)
    model.eval()
    fn, tok = model.get_img_preprocess_fn(), model.get_tokenizer()
    model = model.to(0)
    ds = MBEIRInferenceOnlyDataset(cfg.mbeir_data_dir, queries, cfg.data_config.query_instruct_path, fn,
                                   enable_query_instruct=True, print_config=False)
    col = MBEIRInferenceOnlyCollator(tok, tuple(map(int, str(cfg.data_config.image_size).split(","))))
    loader = DataLoader(ds, batch_size=cfg.dataloader_config.batch_size, shuffle=False, collate_fn=col)
    emb, _ = mbeir_embedder.generate_embeds_and_ids_for_dataset_with_gather(model, loader, 0, use_fp16=True)
    return emb


def _query_dicts(tuples):
    task = {"text -> image": 0, "text -> text": 1, "text -> image,text": 2, "image -> text": 3, "image -> image": 4,
            "image -> image,text": 5, "image,text -> text": 6, "image,text -> image": 7, "image,text -> image,text": 8}
    return [{"qid": f"9:{i + 1}", "query_modality": m, "query_txt": t, "query_img_path": p, "task_id": task[f"{m} -> {c}"],
             "candidate_modality": c} for i, (m, t, p, c) in enumerate(tuples)]


def _results(uniir_dir, kind, results_dir_name="retrieval_results"):
    base = os.path.join(uniir_dir, results_dir_name, "CLIP_SF/Instruct" if kind == "clip" else "BLIP_FF/Instruct")
    run = open(os.path.join(base, "run_files", "mbeir_toy_single_pool_val_k10_run.txt"), "rb").read()
    path = os.path.join(base, "retrieved_candidates", "mbeir_toy_single_pool_val_k10_retrieved.jsonl")
    raw = open(path, "rb").read() if os.path.exists(path) else None
    return run, raw


def _check_unirag(tmp_path, kind, monkeypatch):
    from oracle import c_oracle
    import mbeir_retriever
    data_dir, uniir_dir, cfgs, cands, queries = _prepare(tmp_path, kind, monkeypatch)
    by_did = {c["did"]: c for c in cands}
    plain = mbeir_retriever.run_retrieval(_load(cfgs["retrieval"], uniir_dir, data_dir), None)
    run_plain, raw_none = _results(uniir_dir, kind)
    assert raw_none is None
    shutil.rmtree(os.path.join(uniir_dir, "retrieval_results"))
    rcfg = _load(cfgs["retrieval"], uniir_dir, data_dir)
    rcfg.retrieval_config.raw_retrieval = True
    ecfg = _load(cfgs["embed"], uniir_dir, data_dir)
    rag = mbeir_retriever.run_retrieval(rcfg, ecfg)
    run_rag, raw = _results(uniir_dir, kind)
    assert run_rag == run_plain
    strip = lambda rows: [{k: v for k, v in r.items() if k != "Dataset"} for r in rows]     # noqa: E731
    assert strip(rag) == strip(plain)
    assert {r["Dataset"] for r in plain} == {"toy"} and {r["Dataset"] for r in rag} == {"MSCOCO"}    # the reference's quirk
    lines = raw.decode().split("\n")
    assert lines[-1] == "" and len(lines) == N_QUERY + 1
    recs = [json.loads(l) for l in lines[:-1]]
    assert [json.dumps(r) + "\n" for r in recs] == [l + "\n" for l in lines[:-1]]
    run_ids = [l.split()[2] for l in run_rag.decode().strip().split("\n")]
    comp_queries, owners = [], []
    for qi, rec in enumerate(recs):
        assert rec["query"] == queries[qi]
        assert rec["candidates"] == [by_did[d] for d in run_ids[qi * 10:(qi + 1) * 10]]
        assert list(rec) == ["query", "candidates", "complement_candidates"]
        for c in rec["candidates"]:
            if c["modality"] in ("text", "image"):
                other = "image" if c["modality"] == "text" else "text"
                comp_queries.append((c["modality"], c["txt"], c["img_path"], other))
                owners.append(qi)
    assert comp_queries and any(c["modality"] == "image,text" for r in recs for c in r["candidates"])
    # restatement: embed the complement queries independently, exact top-10 from the C oracle, the selection rule
    base = os.path.join(uniir_dir, "embed", "CLIP_SF/Instruct" if kind == "clip" else "BLIP_FF/Instruct", "cand_pool")
    pool = np.load(os.path.join(base, "mbeir_toy_cand_pool_embed.npy"))
    pool_ids = np.load(os.path.join(base, "mbeir_toy_cand_pool_ids.npy"))
    qemb = _embed_independently(ecfg, _query_dicts(comp_queries))
    _, top = c_oracle.topk(pool, pool_ids, qemb, 10)
    want = [[] for _ in recs]
    for n, (cq, qi) in enumerate(zip(comp_queries, owners)):
        q = queries[qi]
        pick = None
        for h in top[n]:
            c = by_did[f"9:{int(h) % 10_000_000}"]
            if c["modality"] != cq[3]:
                continue
            if c.get("img_path") and c.get("img_path") != q["query_img_path"]:
                pick = c
                break
            if c.get("txt") and c.get("txt") != q["query_txt"]:
                pick = c
                break
        want[qi].append(pick)
    assert [r["complement_candidates"] for r in recs] == want
    return data_dir, uniir_dir, cfgs, by_did


def test_unirag_raw_retrieval_clip_sf(tmp_path, monkeypatch):
    data_dir, uniir_dir, cfgs, by_did = _check_unirag(tmp_path, "clip", monkeypatch)
    # a standalone InteractiveRetriever: text, image and image+text queries against the C oracle's top-k
    from oracle import c_oracle
    from interactive_retriever import InteractiveRetriever
    ecfg = _load(cfgs["embed"], uniir_dir, data_dir)
    index = os.path.join(uniir_dir, "index", "CLIP_SF/Instruct", "cand_pool", "mbeir_toy_cand_pool.index")
    ir = InteractiveRetriever(index, os.path.join(data_dir, "cand_pool", "mbeir_toy_cand_pool.jsonl"), "MSCOCO", ecfg)
    tuples = [("text", "red dog river", None, "image"), ("image", None, "img/c0.png", "text"),
              ("image,text", "blue car", "img/c2.png", "image,text")]
    ir.add_queries(tuples[:2])
    ir.add_queries(tuples[2:])
    assert [q["qid"] for q in ir.queries] == ["9:1", "9:2", "9:3"]
    got = ir.retrieve(k=5, batch_size=2)
    base = os.path.join(uniir_dir, "embed", "CLIP_SF/Instruct", "cand_pool")
    _, top = c_oracle.topk(np.load(os.path.join(base, "mbeir_toy_cand_pool_embed.npy")),
                           np.load(os.path.join(base, "mbeir_toy_cand_pool_ids.npy")),
                           _embed_independently(ecfg, _query_dicts(tuples)), 5)
    assert got == [[by_did[f"9:{int(h) % 10_000_000}"] for h in row] for row in top]
    assert not os.path.exists("interactive_queries_embed.npy")


def test_unirag_raw_retrieval_blip_ff_small(tmp_path, monkeypatch):
    _check_unirag(tmp_path, "blip", monkeypatch)


def _rank_worker(rank, world, port, data_dir, uniir_dir, cfgs, q):
    import torch.distributed as dist
    for p in (ROOT, SRC, os.path.join(SRC, "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _patch_models("clip", uniir_dir)
        import mbeir_retriever
        rcfg = _load(cfgs["retrieval"], uniir_dir, data_dir, distributed=True)
        rcfg.retrieval_config.raw_retrieval = True
        rcfg.retrieval_config.results_dir_name = "results_2rank"
        res = mbeir_retriever.run_retrieval(rcfg, _load(cfgs["embed"], uniir_dir, data_dir, distributed=True))
        q.put((rank, json.dumps(res)))
    finally:
        dist.destroy_process_group()


def test_unirag_two_ranks_write_the_bytes_of_one(tmp_path, monkeypatch):
    import mbeir_retriever
    data_dir, uniir_dir, cfgs, _, _ = _prepare(tmp_path, "clip", monkeypatch)
    rcfg = _load(cfgs["retrieval"], uniir_dir, data_dir)
    rcfg.retrieval_config.raw_retrieval = True
    one = mbeir_retriever.run_retrieval(rcfg, _load(cfgs["embed"], uniir_dir, data_dir))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, 29563, data_dir, uniir_dir, cfgs, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = dict(q.get(timeout=300) for _ in range(2))
    finally:
        for p in procs:
            p.join(timeout=120)
            if p.is_alive():          # a rank that failed leaves its peer waiting in a collective
                p.terminate()
                p.join(timeout=30)
    assert [p.exitcode for p in procs] == [0, 0]
    assert json.loads(got[0]) == json.loads(got[1]) == json.loads(json.dumps(one))
    run1, raw1 = _results(uniir_dir, "clip")
    run2, raw2 = _results(uniir_dir, "clip", "results_2rank")
    assert raw1 is not None and run2 == run1 and raw2 == raw1
