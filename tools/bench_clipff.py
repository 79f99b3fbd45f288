#!/usr/bin/env python
"""Secondary benchmark: CLIP_FF ViT-L/14 train step (towers without pooling -> 2-layer T5 fusion over 334 tokens ->
mean pooling -> InfoNCE), synthetic data, one MI355X.   python tools/bench_clipff.py --pairs 256 --steps 4
--model "ViT-L/14@336px": the 336-pixel towers, 654 fused tokens (the streaming relative-bias attention).  --embed-items N adds a
second JSON line: the eval-mode embedding rate over batches of N items (encode_mbeir_batch).  UNIIR_RECOMPUTE_BLOCKS=1 is named in
the line when it is set."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="ViT-L/14")
    ap.add_argument("--embed-items", type=int, default=0)
    a = ap.parse_args()
    from bench import synth_batch
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from uniir_amd.clip_model import CLIP_CONFIGS
    from uniir_amd.trainer import NativeTrainer
    dev = torch.device("cuda:0")
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=True), data_config=SimpleNamespace(in_batch_neg_num=0))
    model = CLIPFeatureFusion(a.model, device=dev, config=config)
    tr = NativeTrainer(model, lr=1e-5, t_total=1000)
    batch = synth_batch(CLIP_CONFIGS[a.model], a.pairs, 2023, dev)
    for _ in range(a.warmup):
        out = tr.train_step(batch)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = tr.train_step(batch)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / a.steps
    recompute = os.environ.get("UNIIR_RECOMPUTE_BLOCKS", "0")
    print(json.dumps({"metric": f"train_pairs_per_s (CLIP_FF {a.model})", "value": a.pairs / dt, "unit": "pairs/s",
                      "ms_per_step": dt * 1e3, "pairs": a.pairs, "loss": float(out["loss"].detach()),
                      "peak_mem_GB": torch.cuda.max_memory_allocated() / 2**30, "recompute_blocks": recompute}), flush=True)
    if a.embed_items:
        model.eval()
        items = {k: (v[:a.embed_items] if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        n = items["txt_batched"].shape[0]
        items["did_list"] = list(range(n))
        with torch.no_grad():
            model(items, encode_mbeir_batch=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                model(items, encode_mbeir_batch=True)
            torch.cuda.synchronize()
        de = (time.perf_counter() - t0) / a.steps
        print(json.dumps({"metric": f"embed_items_per_s (CLIP_FF {a.model})", "value": n / de, "unit": "items/s",
                          "ms_per_batch": de * 1e3, "items": n}), flush=True)


if __name__ == "__main__":
    main()
