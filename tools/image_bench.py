#!/usr/bin/env python
"""Input-pipeline micro-benchmark: the device image transform (uniir_image_preprocess, 500 x 375 RGB -> 3 x 224 x 224 fp32,
CLIP geometry) against the same transform with Pillow on one host core.
    python tools/image_bench.py [--images 512]
With --batched it then compares the per-image path (clip_front.preprocess_on_device) with the batched one
(clip_front.PackedImages -> uniir_image_preprocess_batch) on the same box: two shapes (whole image + centre crop; BLIP-style random
boxes and flips), two cases ((a) bytes resident in HBM, (b) from pinned host memory, copy included), the two paths alternating, two
runs each; the table goes to --out as well.
    python tools/image_bench.py --batched [--out profiles/image_batch.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from uniir_amd import clip_front  # noqa: E402


def _timed(fn, reps):
    """one warm-up pass, then `reps` passes between two device synchronisations -> seconds per pass"""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def batched_ab(images, out_path, reps_per_image=5, reps_batched=20):
    import random

    from uniir_amd.blip_front import RawBlipTransform
    n, dev = 224, torch.device("cuda")
    rng = np.random.default_rng(0)
    host = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8) for _ in range(images)]
    random.seed(0)
    draws = [RawBlipTransform(n).draw(500, 375) for _ in range(images)]
    shapes = {
        "whole image, centre crop (CLIP)": ([torch.from_numpy(x) for x in host], None, True),
        # the per-image entry point has no box and no flip: it gets the boxes cut out beforehand (not timed) and resizes them to
        # n x n unflipped -- the same source pixels and output size as the batched call, which cuts and mirrors on the device
        "BLIP-style random boxes and flips": ([torch.from_numpy(np.ascontiguousarray(x[t:t + bh, le:le + bw]))
                                               for x, (le, t, bw, bh, f) in zip(host, draws)],
                                              [(le, t, bw, bh, n, n, 0, 0, f) for le, t, bw, bh, f in draws], False),
    }
    lines = [f"Device image transform, {images} images of 500 x 375 -> 3 x {n} x {n} fp32: the per-image path (preprocess_on_device: one copy",
             "and up to five launches per image) and the batched path (PackedImages.run: one copy, three launches per batch) on ONE box,",
             f"alternating (per-image, batched, per-image, batched); a run = one warm-up pass + {reps_per_image} (per-image) / {reps_batched} (batched)",
             "timed passes between device synchronisations.  images/s (us per image); spread = |per-image run 1 - run 2|.", ""]
    out_a, out_b = torch.empty(images, 3, n, n, device=dev), torch.empty(images, 3, n, n, device=dev)
    for what, (per_image_src, geoms, center_crop) in shapes.items():
        packed_src = [torch.from_numpy(x) for x in host]
        t0 = time.perf_counter()
        packed = clip_front.PackedImages(packed_src, geoms, n, pin=True)
        pack_s = time.perf_counter() - t0
        blob = packed.blob.to(dev)
        resident = [x.to(dev) for x in per_image_src]
        pinned = [x.pin_memory() for x in per_image_src]
        cases = {
            "(a) bytes resident in HBM": (lambda: clip_front.preprocess_on_device(resident, n, dev, center_crop=center_crop, out=out_a),
                                          lambda: packed.run(dev, out=out_b, blob=blob)),
            "(b) from pinned host memory, copy included": (
                lambda: clip_front.preprocess_on_device(pinned, n, dev, center_crop=center_crop, out=out_a),
                lambda: packed.run(dev, out=out_b)),
        }
        lines.append(f"{what}   [packing {images} images into the pinned buffer on the host: {pack_s * 1e3:.1f} ms, not in the figures]")
        for case, (per_image, batched) in cases.items():
            t = {"p": [], "b": []}
            for _ in range(2):
                t["p"].append(_timed(per_image, reps_per_image))
                t["b"].append(_timed(batched, reps_batched))
            if geoms is None:
                same = bool(torch.equal(out_a, out_b))
            else:       # the per-image path did not mirror: compare with the flip undone
                flip = torch.tensor([g[8] for g in geoms], device=dev, dtype=torch.bool)
                same = bool(torch.equal(torch.where(flip[:, None, None, None], out_b.flip(3), out_b), out_a))
            f = lambda s: f"{images / s:9.0f} ({s / images * 1e6:6.2f} us)"
            mp, mb = sum(t["p"]) / 2, sum(t["b"]) / 2
            lines.append(f"  {case:44s} per-image {f(t['p'][0])} {f(t['p'][1])}  spread {abs(t['p'][0] - t['p'][1]) / images * 1e6:5.2f} us"
                         f" | batched {f(t['b'][0])} {f(t['b'][1])} | batched / per-image time {mb / mp:.3f}  outputs equal: {same}")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--batched", action="store_true", help="also compare the per-image and the batched path")
    ap.add_argument("--out", default="", help="with --batched: write the table to this file as well")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    dev = torch.device("cuda")
    host = [rng.integers(0, 256, (375, 500, 3), dtype=np.uint8) for _ in range(args.images)]
    resident = [torch.from_numpy(x).to(dev) for x in host]
    out = torch.empty(args.images, 3, 224, 224, device=dev)
    for src, what in ((resident, "uint8 already in HBM"), (host, "uint8 in pageable host memory (H2D included)")):
        clip_front.preprocess_on_device(src[:8], 224, dev, out=out[:8])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        clip_front.preprocess_on_device(src, 224, dev, out=out)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"device transform, {what}: {args.images / dt:8.0f} images/s ({dt / args.images * 1e6:6.1f} us per image)")
    from PIL import Image
    fn = clip_front._preprocess(224)
    pil = [Image.fromarray(x, "RGB") for x in host[:64]]
    t0 = time.perf_counter()
    for im in pil:
        fn(im)
    dt = time.perf_counter() - t0
    print(f"Pillow + torch on one host core: {64 / dt:8.0f} images/s ({dt / 64 * 1e6:6.1f} us per image)")
    if args.batched:
        batched_ab(args.images, args.out)


if __name__ == "__main__":
    main()
