"""BLIP_FF training-step time with BLIPFeatureFusion.pool_last_layer off / on (dev tool; profiles/blip_pooled_last_layer.txt).
One process per arm, the flag through UNIIR_BLIP_POOL_LAST_LAYER:
  --vit large : bench.py's own BLIP_FF block (bench.bench_blip_ff, config 5: ViT-L/16 @224 + MED BERT-base, 256 pairs, queue 57344,
                100 text tokens, train-mode dropout), unmodified -- the number `bench.py --full` reports as blip_ff_large;
  --vit base  : the same step with ViT-B/16 (the base YAMLs), timed here per step (median).
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402


def base_step(dev, pairs, steps, warmup, queue=57344, length=100):
    from uniir_amd.blip_model import BLIPFeatureFusion
    from uniir_amd.trainer import NativeAdamW
    model = BLIPFeatureFusion(med_config={}, vit="base", queue_size=queue, momentum=0.995,
                              config=types.SimpleNamespace(tokenizer_max_length=length)).to(dev)
    model.check_masks = False
    opt = NativeAdamW(model, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, allreduce=False)
    batches = [bench._blip_synth(pairs, length, 30524, s, dev) for s in range(2)]
    times = []
    for i in range(warmup + steps):
        b = batches[i % 2]
        m = b["txt_batched"].attention_mask
        if hasattr(m, "_uniir_pack"):
            del m._uniir_pack
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opt.zero_grad()
        out = model(b, alpha=0.4)
        out["loss"].backward()
        opt.step()
        torch.cuda.synchronize()
        if i >= warmup:
            times.append((time.perf_counter() - t0) * 1e3)
    return {"ms_per_step": round(statistics.median(times), 2), "min": round(min(times), 2), "max": round(max(times), 2),
            "final_loss": round(float(out["loss"]), 4), "path_log": model.path_log[-1:], "text_rows": model.last_text_rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vit", choices=("large", "base"), default="large")
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.vit == "large":
        rec = bench.bench_blip_ff(dev, pairs=a.pairs, steps=a.steps, warmup=a.warmup)
        rec = {k: rec[k] for k in ("ms_per_step", "value", "final_loss", "padded_rows")}
    else:
        rec = base_step(dev, a.pairs, a.steps, a.warmup)
    rec.update(vit=a.vit, pairs=a.pairs, steps=a.steps, pool_last_layer=os.environ.get("UNIIR_BLIP_POOL_LAST_LAYER", "0"))
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
