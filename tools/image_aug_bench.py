#!/usr/bin/env python
"""Micro-benchmark of the device RandomAugment: for 256 images of 500 x 375 with BLIP-style random boxes and flips, at 224 and at
384 pixels, bytes resident in HBM, the time of
  (1) uniir_image_preprocess_batch            (the call without augmentation),
  (2) uniir_image_preprocess_batch_aug        with an all-Identity table of two slots,
  (3) uniir_image_preprocess_batch_aug        with tables drawn by RandAugmentDraw(2, 5),
the three alternating on one box, several runs each; then the numpy restatement (uniir_amd/randaugment.apply_ops -- NOT OpenCV) of
the same drawn ops on one host core.
    python tools/image_aug_bench.py [--out profiles/image_randaugment.txt]"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uniir_amd import clip_front, randaugment  # noqa: E402
from uniir_amd.blip_front import RawBlipTransform  # noqa: E402


def _timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rng = np.random.default_rng(0)
    host = [torch.from_numpy(rng.integers(0, 256, (375, 500, 3), dtype=np.uint8)) for _ in range(args.images)]
    lines = [f"Device RandomAugment, {args.images} images of 500 x 375, BLIP-style random boxes and flips -> 3 x n x n fp32, bytes resident in HBM.",
             "plain = uniir_image_preprocess_batch (3 launches); identity = uniir_image_preprocess_batch_aug with an all-Identity table of",
             "two slots (8 launches); drawn = the same with tables drawn by RandAugmentDraw(2, 5).  One box, the three alternating",
             f"(plain, identity, drawn, plain, ...); a run = one warm-up pass + {args.reps} timed passes between device synchronisations.",
             "us per batch, every run listed; spread = max - min of the runs.", ""]
    for n in (224, 384):
        random.seed(0)
        np.random.seed(0)
        tf = RawBlipTransform(n, randaugment=(2, 5))
        draws = [tf.draw(500, 375) for _ in host]
        geoms = [(le, t, bw, bh, n, n, 0, 0, f) for le, t, bw, bh, f in draws]
        ops = [tf.randaugment.draw() for _ in host]
        packs = {"plain": clip_front.PackedImages(host, geoms, n),
                 "identity": clip_front.PackedImages(host, geoms, n, augs=[[("Identity", 0.0)] * 2] * len(host)),
                 "drawn": clip_front.PackedImages(host, geoms, n, augs=ops)}
        blobs = {k: p.blob.to(dev) for k, p in packs.items()}
        outs = {k: torch.empty(len(host), 3, n, n, device=dev) for k in packs}
        times = {k: [] for k in packs}
        for _ in range(args.runs):
            for k, p in packs.items():
                times[k].append(_timed(lambda: p.run(dev, out=outs[k], blob=blobs[k]), args.reps))
        same = bool(torch.equal(outs["plain"], outs["identity"]))
        used = sorted({name for o in ops for name, _ in o})
        lines.append(f"n = {n}   (identity output == plain output: {same}; ops drawn: {', '.join(used)})")
        for k, ts in times.items():
            us = [t * 1e6 for t in ts]
            lines.append(f"  {k:9s} " + " ".join(f"{u:9.1f}" for u in us) + f"   mean {sum(us) / len(us):9.1f} us  spread {max(us) - min(us):7.1f} us"
                         f"   {len(host) / (sum(ts) / len(ts)):10.0f} images/s")
        # the restatement on one host core, on the resized bytes the device works on
        rows = [outs["plain"][i] for i in range(8)]
        mean, std = torch.tensor(clip_front._MEAN, device=dev).view(3, 1, 1), torch.tensor(clip_front._STD, device=dev).view(3, 1, 1)
        u8 = [((r * std + mean) * 255).round().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().cpu().numpy() for r in rows]
        torch.set_num_threads(1)
        t0, done = time.perf_counter(), 0
        for rep in range(4):
            for i in range(len(host)):
                randaugment.apply_ops(u8[i % 8], ops[i])
                done += 1
        dt = time.perf_counter() - t0
        lines.append(f"  numpy restatement of the drawn ops (not OpenCV), one host core: {done / dt:8.0f} images/s ({dt / done * 1e6:7.1f} us per image)")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
