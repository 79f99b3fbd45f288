#!/usr/bin/env python
"""Times the UniRAG `--enable_retrieval` stage (mbeir_retriever.run_retrieval with raw_retrieval and
retrieve_image_text_pairs) on a synthetic M-BEIR tree, in two schedules of the same code:
  (a) this implementation: one model per process, each candidate jsonl parsed once, query embeddings kept in HBM, the
      pool shards uploaded once;
  (b) the reference's schedule (src/common/interactive_retriever.py, mbeir_retriever.py:451-466): the model rebuilt for
      every dataset, the candidate jsonl parsed twice per dataset, the complement-query embeddings written to
      ./interactive_queries_embed.npy and read back, the index re-read and re-uploaded for every search.
Synthetic tree: a union pool of --pool records (40 % text, 40 % image, 20 % image+text; --images distinct PNG files),
--datasets x --queries text queries, Recall@1/5/10, random pool / query embeddings written as the embed stage would, and
a random-init CLIP_SF ViT-B/32 for the complement queries (a toy word-hash tokenizer: the BPE vocabulary is not shipped).
Each schedule runs in a fresh process, alternating, --repeats times; one JSON line per run and a summary line.
    python tools/bench_unirag.py --workdir /tmp/unirag_bench [--pool 200000 --datasets 2 --queries 1000 --repeats 2]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "uniir_amd", "src")
DIM = 512


def _toy_tokenize(texts, context_length=77, truncate=True):
    import torch
    out = torch.zeros(len(texts), context_length, dtype=torch.int32)
    for i, t in enumerate(texts):
        ids = [49406] + [1 + (sum(map(ord, w)) % 49000) for w in t.split()][: context_length - 2] + [49407]
        out[i, : len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return out


def make_tree(work, n_pool, n_ds, n_q, n_img, seed=0):
    from PIL import Image
    for p in (SRC, os.path.join(SRC, "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from data.preprocessing.utils import hash_did, hash_qid
    rng = np.random.default_rng(seed)
    data, uniir = os.path.join(work, "mbeir"), os.path.join(work, "uniir")
    for sub in ("img", "test", "cand_pool", "instructions", "qrels/test"):
        os.makedirs(os.path.join(data, sub), exist_ok=True)
    for i in range(n_img):
        Image.fromarray(rng.integers(0, 255, (256, 320, 3), dtype=np.uint8)).save(os.path.join(data, f"img/i{i}.png"))
    words = np.array("red blue dog cat tree car river house bird stone cloud road green small old boat".split())
    mods = rng.choice(["text", "image", "image,text"], size=n_pool, p=[0.4, 0.4, 0.2])
    with open(os.path.join(data, "cand_pool", "mbeir_union_test_cand_pool.jsonl"), "w") as f:
        for i, m in enumerate(mods):
            rec = {"txt": " ".join(rng.choice(words, 6)) if "text" in m else None,
                   "img_path": f"img/i{rng.integers(n_img)}.png" if "image" in m else None, "modality": str(m),
                   "did": f"{i % 10}:{i // 10 + 1}", "src_content": None}
            f.write(json.dumps(rec) + "\n")
    dids = np.array([hash_did(f"{i % 10}:{i // 10 + 1}") for i in range(n_pool)], dtype=np.int64)
    embed = os.path.join(uniir, "embed", "CLIP_SF/Instruct")
    os.makedirs(os.path.join(embed, "cand_pool"), exist_ok=True)
    os.makedirs(os.path.join(embed, "test"), exist_ok=True)
    np.save(os.path.join(embed, "cand_pool", "mbeir_union_cand_pool_embed.npy"),
            rng.standard_normal((n_pool, DIM)).astype(np.float16))
    np.save(os.path.join(embed, "cand_pool", "mbeir_union_cand_pool_ids.npy"), dids)
    names = [f"ds{d}" for d in range(n_ds)]
    for d, name in enumerate(names):
        qids = [f"{d}:{i + 1}" for i in range(n_q)]
        with open(os.path.join(data, "test", f"mbeir_{name}_test.jsonl"), "w") as f, \
                open(os.path.join(data, "qrels/test", f"mbeir_{name}_test_qrels.txt"), "w") as g:
            for q in qids:
                pos = int(rng.integers(n_pool))
                f.write(json.dumps({"qid": q, "query_txt": " ".join(rng.choice(words, 5)), "query_img_path": None,
                                    "query_modality": "text", "query_src_content": None, "pos_cand_list": [], "neg_cand_list": [],
                                    "task_id": 0}) + "\n")
                g.write(f"{q} 0 {pos % 10}:{pos // 10 + 1} 1 0\n")
        np.save(os.path.join(embed, "test", f"mbeir_{name}_test_embed.npy"), rng.standard_normal((n_q, DIM)).astype(np.float16))
        np.save(os.path.join(embed, "test", f"mbeir_{name}_test_ids.npy"),
                np.array([hash_qid(q) for q in qids], dtype=np.int64))
    with open(os.path.join(data, "instructions", "query_instructions.tsv"), "w") as f:
        f.write("query_modality\tcand_modality\tdataset_name\tdataset_id\tprompt_1\tprompt_2\n")
        f.write("text\timage\tMSCOCO\t9\tFind me an everyday image that matches the given caption.\tShow me an image.\n")
        f.write("image\ttext\tMSCOCO\t9\tFind a caption for the image.\tDescribe the image.\n")
    common = {"experiment": {"instruct_status": "Instruct", "path_suffix": "CLIP_SF/Instruct/"},
              "model": {"name": "CLIPScoreFusion", "short_name": "CLIP_SF", "clip_vision_model_name": "ViT-B/32",
                        "pretrained_clip_model_dir": "checkpoint/CLIP/",
                        "ckpt_config": {"ckpt_dir": "checkpoint/bench/", "ckpt_name": "clip_sf_b32.pth"}},
              "seed": 2023, "dist_config": {"dist_url": "env://"}}
    embed_cfg = dict(common, embed_config={"embed_dir_name": "embed", "use_fp16": True},
                     dataloader_config={"num_workers": 8, "batch_size": 256},
                     data_config={"image_size": "224, 224", "enable_query_instruct": True,
                                  "query_instruct_path": "instructions/query_instructions.tsv"})
    retr_cfg = dict(common, retrieval_config={
        "embed_dir_name": "embed", "index_dir_name": "index", "results_dir_name": "retrieval_results", "qrel_dir_name": "qrels",
        "query_dir_name": "", "candidate_dir_name": "cand_pool", "write_to_tsv": True, "raw_retrieval": True,
        "retrieve_image_text_pairs": True,
        "test_datasets_config": {"enable_retrieve": True, "datasets_name": names, "correspond_cand_pools_name": ["UNION"] * n_ds,
                                 "correspond_qrels_name": names, "correspond_metrics_name": ["Recall@1, Recall@5, Recall@10"] * n_ds}})
    index_cfg = dict(common, index_config={"faiss_config": {"dim": DIM}, "embed_dir_name": "embed", "index_dir_name": "index",
                                           "cand_pools_config": {"enable_idx": True, "cand_pools_name_to_idx": ["UNION"]}})
    for name, cfg in (("embed", embed_cfg), ("retrieval", retr_cfg), ("index", index_cfg)):
        with open(os.path.join(work, f"{name}.json"), "w") as f:
            json.dump(cfg, f)
    return data, uniir


def _setup(work):
    for p in (ROOT, SRC, os.path.join(SRC, "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["UNIIR_ALLOW_RANDOM_INIT"] = "1"        # no pretrained file: the checkpoint below holds the weights
    from config import OmegaConf
    from uniir_amd import clip_front
    clip_front.tokenize = _toy_tokenize
    cfgs = {}
    for name in ("embed", "retrieval", "index"):
        c = OmegaConf.create(json.load(open(os.path.join(work, f"{name}.json"))))
        c.uniir_dir, c.mbeir_data_dir = os.path.join(work, "uniir"), os.path.join(work, "mbeir")
        c.dist_config.gpu_id, c.dist_config.distributed_mode = 0, False
        cfgs[name] = c
    return cfgs


def prepare(work):
    """the random-init ViT-B/32 checkpoint and the index file (not timed)"""
    import torch
    cfgs = _setup(work)
    from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
    import mbeir_retriever
    torch.manual_seed(0)
    m = CLIPScoreFusion(model_name="ViT-B/32", device="cuda:0")
    ck = os.path.join(cfgs["embed"].uniir_dir, "checkpoint/bench")
    os.makedirs(ck, exist_ok=True)
    torch.save({"model": m.state_dict()}, os.path.join(ck, "clip_sf_b32.pth"))
    mbeir_retriever.create_index(cfgs["index"])


def reference_schedule():
    """patch the caches and the in-HBM hand-off away: the reference's per-dataset rebuild / re-parse / .npy round trip"""
    import interactive_retriever as ir
    import mbeir_retriever as mr
    load = ir.load_candidates_by_did

    def parse_every_time(path):
        ir._CAND_CACHE.clear()
        return load(path)

    ir.load_candidates_by_did = mr.load_candidates_by_did = parse_every_time
    init = ir.InteractiveRetriever.__init__

    def rebuild(self, *a, **k):
        ir._MODEL_CACHE.clear()
        init(self, *a, **k)

    ir.InteractiveRetriever.__init__ = rebuild
    embed = ir.InteractiveRetriever._embed_queries

    def via_npy(self):
        np.save("interactive_queries_embed.npy", embed(self).cpu().numpy())
        return np.load("interactive_queries_embed.npy")

    ir.InteractiveRetriever._embed_queries = via_npy
    search = mr.search_embeddings

    def reupload(*a, **k):
        mr._SHARD_CACHE.clear()
        return search(*a, **k)

    mr.search_embeddings = reupload
    retrieve = ir.InteractiveRetriever.retrieve

    def retrieve_and_remove(self, *a, **k):
        out = retrieve(self, *a, **k)
        if os.path.exists("interactive_queries_embed.npy"):
            os.remove("interactive_queries_embed.npy")
        return out

    ir.InteractiveRetriever.retrieve = retrieve_and_remove


def run(work, mode):
    import torch
    cfgs = _setup(work)
    import mbeir_retriever
    import interactive_retriever
    if mode == "reference_schedule":
        reference_schedule()
    phases = {}

    def timed(owner, name, label):          # wall time per phase, the device drained at both ends
        f = getattr(owner, name)

        def wrapper(*a, **k):
            torch.cuda.synchronize()
            t = time.perf_counter()
            try:
                return f(*a, **k)
            finally:
                torch.cuda.synchronize()
                phases[label] = phases.get(label, 0.0) + time.perf_counter() - t

        setattr(owner, name, wrapper)

    timed(interactive_retriever, "_query_embedder", "model_build")
    timed(interactive_retriever, "load_candidates_by_did", "parse_candidates")
    timed(mbeir_retriever, "load_candidates_by_did", "parse_candidates")
    timed(interactive_retriever.InteractiveRetriever, "_embed_queries", "embed_complement_queries")
    timed(mbeir_retriever, "search_embeddings", "search")
    timed(mbeir_retriever, "write_retrieved_jsonl", "write_jsonl")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    results = mbeir_retriever.run_retrieval(cfgs["retrieval"], cfgs["embed"])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out_dir = os.path.join(cfgs["retrieval"].uniir_dir, "retrieval_results", "CLIP_SF/Instruct", "retrieved_candidates")
    n_comp = 0
    for name in sorted(os.listdir(out_dir)):
        with open(os.path.join(out_dir, name)) as f:
            n_comp += sum(len(json.loads(line)["complement_candidates"]) for line in f)
    return {"mode": mode, "seconds": round(dt, 3), "phases_s": {k: round(v, 3) for k, v in sorted(phases.items())},
            "complement_queries": n_comp, "results": results}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workdir", required=True)
    ap.add_argument("--pool", type=int, default=200_000)
    ap.add_argument("--datasets", type=int, default=2)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print("BENCH_UNIRAG " + json.dumps(run(a.workdir, a.child)), flush=True)
        return
    if a.child is None and not os.path.exists(os.path.join(a.workdir, "retrieval.json")):
        t0 = time.perf_counter()
        make_tree(a.workdir, a.pool, a.datasets, a.queries, a.images)
        subprocess.check_call([sys.executable, "-c", f"import sys; sys.path.insert(0, {os.path.dirname(__file__)!r}); "
                               f"import bench_unirag as b; b.prepare({a.workdir!r})"])
        print(f"tree + checkpoint + index in {time.perf_counter() - t0:.1f} s", flush=True)
    runs = []
    for _ in range(a.repeats):
        for mode in ("this", "reference_schedule"):          # alternating, each in a fresh process
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--workdir", a.workdir, "--child", mode],
                               capture_output=True, text=True, cwd=a.workdir)
            line = [l for l in p.stdout.splitlines() if l.startswith("BENCH_UNIRAG ")]
            if p.returncode != 0 or not line:
                sys.stderr.write(p.stdout[-4000:] + p.stderr[-4000:])
                raise SystemExit(f"{mode} run failed with exit status {p.returncode}")
            r = json.loads(line[0][len("BENCH_UNIRAG "):])
            print(json.dumps({k: v for k, v in r.items() if k != "results"}), flush=True)
            runs.append(r)
    same = all(r["results"] == runs[0]["results"] for r in runs)
    best = {m: min(r["seconds"] for r in runs if r["mode"] == m) for m in ("this", "reference_schedule")}
    print(json.dumps({"metric": "UniRAG --enable_retrieval stage seconds (lower is better)", "pool": a.pool,
                      "datasets": a.datasets, "queries_per_dataset": a.queries, "best_s": best,
                      "speedup_vs_reference_schedule": round(best["reference_schedule"] / best["this"], 3),
                      "results_identical": same}))


if __name__ == "__main__":
    main()
