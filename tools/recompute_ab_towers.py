"""Same-process A/B of block recomputation in the per-op towers (uniir_amd/resblocks.py, recompute_from) on one MI355X:

  blip_ff  BLIP_FF large (tools/bench_blip.py's model, batches and optimizer) with vit_ckpt_layer 0, 12 and 24 under vit_grad_ckpt
           (BLIPFeatureFusion.vit_recompute_from = 24, 12, 0): none, the upper half and all of the 24 ViT blocks recomputed
  clip_ff  CLIP_FF ViT-L/14 (tools/bench_clipff.py's model, batch and trainer) with CLIP.recompute_blocks off and on

The arms alternate in blocks of timed steps in one process; every block starts with one warm-up step, every step is timed with device
events, and torch's peak is taken per block.  From the peak and what is allocated between steps (weights, optimizer state, queues) the
report computes the pairs that would fit a 288 GB device -- arithmetic, nothing is run out of memory.
The arm "stored" leaves the model exactly as its constructor built it, so  --arms stored  also runs on a tree that has no recomputation
(stored mode of two trees against each other: alternate the two commands and compare the spreads).

    python tools/recompute_ab_towers.py --model blip_ff [--pairs 256] [--blocks 2] [--steps 4] [--arms ckpt0,ckpt12,ckpt24] [--out FILE]
    python tools/recompute_ab_towers.py --model clip_ff [--pairs 256] [--arms off,recompute] [--out FILE] [--append]
"""
import argparse
import os
import statistics
import sys
import time
import types
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

DEVICE_BYTES = 288e9
MARGIN_BYTES = 16 * 2**30      # kept free in the fit computation: collectives' buffers, the allocator's fragmentation


def timed(fn):
    """milliseconds of fn() on the current stream, by device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def build_blip_ff(pairs, dev):
    import bench_blip
    from uniir_amd.blip_model import BLIPFeatureFusion
    from uniir_amd.trainer import NativeAdamW
    model = BLIPFeatureFusion(med_config={}, vit="large", queue_size=57344, momentum=0.995,
                              config=types.SimpleNamespace(tokenizer_max_length=100)).to(dev)
    model.check_masks = False
    opt = NativeAdamW(model, lr=1e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, allreduce=False)
    batches = [bench_blip.synth(pairs, 100, 30524, s, dev) for s in range(2)]
    count = [0]

    def step():
        opt.zero_grad()
        out = model(batches[count[0] % 2], alpha=0.4)
        out["loss"].backward()
        opt.step()
        count[0] += 1

    def set_arm(arm):
        if arm != "stored":
            from uniir_amd.blip_model import vit_recompute_from
            model.vit_recompute_from = vit_recompute_from(model.vit_cfg["depth"], True, int(arm[len("ckpt"):]))

    def describe(arm):
        return "as constructed" if arm == "stored" else f"vit_recompute_from = {model.vit_recompute_from}"

    return "BLIP_FF vit-large/16@224 + MED BERT-base", step, set_arm, describe, lambda: []


def build_clip_ff(pairs, dev):
    from bench import synth_batch
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from uniir_amd.clip_model import CLIP_CONFIGS
    from uniir_amd.trainer import NativeTrainer
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=True), data_config=SimpleNamespace(in_batch_neg_num=0))
    model = CLIPFeatureFusion("ViT-L/14", device=dev, config=config)
    tr = NativeTrainer(model, lr=1e-5, t_total=1000)
    batch = synth_batch(CLIP_CONFIGS["ViT-L/14"], pairs, 2023, dev)
    clip = model.clip_model

    def set_arm(arm):
        if arm != "stored":
            clip.recompute_blocks = arm == "recompute"

    def describe(arm):
        return "as constructed" if arm == "stored" else f"recompute_blocks = {clip.recompute_blocks}"

    return "CLIP_FF ViT-L/14", (lambda: tr.train_step(batch)), set_arm, describe, lambda: list(clip.stash_log)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("blip_ff", "clip_ff"), required=True)
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--blocks", type=int, default=2, help="blocks of timed steps per arm, the arms alternating")
    ap.add_argument("--steps", type=int, default=4, help="timed steps per block (after one warm-up step)")
    ap.add_argument("--arms", default=None, help="blip_ff: stored, ckptN; clip_ff: stored, off, recompute")
    ap.add_argument("--label", default="", help="free text for the header (which tree this is)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--append", action="store_true")
    args = ap.parse_args()
    arms = (args.arms or {"blip_ff": "ckpt0,ckpt12,ckpt24", "clip_ff": "off,recompute"}[args.model]).split(",")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(2023)
    name, step, set_arm, describe, log = (build_blip_ff if args.model == "blip_ff" else build_clip_ff)(args.pairs, dev)
    say(f"# tools/recompute_ab_towers.py: {name}, {args.pairs} pairs, {torch.cuda.get_device_name(0)}, "
        f"{time.strftime('%Y-%m-%d %H:%M:%S %Z')} (this box's clock){' -- ' + args.label if args.label else ''}")
    say(f"# {args.blocks} blocks x {args.steps} timed steps per arm after one warm-up step per block, arms alternating in one process; "
        "device events; ms per step")
    times, peaks, between, what = {a: [] for a in arms}, {a: 0 for a in arms}, {a: 0 for a in arms}, {}
    for blk in range(args.blocks):
        for arm in arms:
            set_arm(arm)
            what[arm] = describe(arm)
            torch.cuda.empty_cache()
            step()                                              # warm-up (first block: lazy buffers, optimizer state)
            torch.cuda.synchronize()
            between[arm] = max(between[arm], torch.cuda.memory_allocated(dev))
            torch.cuda.reset_peak_memory_stats(dev)
            ts = [timed(step) for _ in range(args.steps)]
            times[arm] += ts
            peaks[arm] = max(peaks[arm], torch.cuda.max_memory_allocated(dev))
            say(f"block {blk} {arm:9s} " + " ".join(f"{t:8.2f}" for t in ts))
    say()
    say(f"{'arm':9s} {'setting':26s} {'median ms':>10s} {'min':>9s} {'max':>9s} {'pairs/s':>9s} {'vs first':>9s} {'torch peak bytes':>17s} "
        f"{'between steps':>14s} {'pairs that fit 288 GB':>22s}")
    first = statistics.median(times[arms[0]])
    for arm in arms:
        m = statistics.median(times[arm])
        per_pair = (peaks[arm] - between[arm]) / args.pairs
        fit = int((DEVICE_BYTES - MARGIN_BYTES - between[arm]) // per_pair)
        say(f"{arm:9s} {what[arm]:26s} {m:10.2f} {min(times[arm]):9.2f} {max(times[arm]):9.2f} {args.pairs / m * 1e3:9.1f} "
            f"{100 * (m - first) / first:+8.1f}% {peaks[arm]:17d} {between[arm]:14d} {fit:22d}")
    say(f"# fit: (288e9 - {MARGIN_BYTES} margin - bytes allocated between steps) / ((peak - between steps) / pairs): the step's transient "
        "memory is activations and scales with the pairs (the loss's similarity matrices against the fixed queue included); computed, "
        "not probed")
    for s in log():
        say("# stash_log: " + s)
    say()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
