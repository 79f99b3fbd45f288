"""Timings of the gradient guard on an MI355X (needs the GPU: no fallback).

  (1) uniir_grad_guard (one range, finish kernel included) over N floats against torch's fp32 sum over the same bytes -- the
      "f32 sum read" line of tools/bw_probe.py -- alternating, medians and spread of device-event timings;
  (2) uniir_adamw_step_guarded against uniir_adamw_step on the same five buffers, alternating;
  (3) --step: one CLIP_SF ViT-L/14 train step (the path bench.py times) with the guard on and off, alternating.

usage: python tools/grad_guard_bench.py [--count 427616513] [--reps 30] [--step] [--pairs 128]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))

import torch

if not torch.cuda.is_available():
    raise SystemExit("grad_guard_bench: no GPU; these are device timings and have no CPU form")

from uniir_amd import ops
from uniir_amd.trainer import GradGuard


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3          # us


def alternate(fns, reps, warmup=3):
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(timed(f))
    return out


def line(name, ts, nbytes):
    med = statistics.median(ts)
    print(f"  {name:<28s} median {med:9.1f} us  min {min(ts):9.1f}  max {max(ts):9.1f}  {nbytes / med / 1e6:6.2f} TB/s")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=427_616_513)          # CLIP ViT-L/14's store: 1.71 GB of fp32 gradient
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--pairs", type=int, default=128)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = a.count
    print(f"device {torch.cuda.get_device_name(0)}; count {n} ({4 * n / 1e9:.2f} GB); chunk {ops.grad_guard_chunk()}")

    # ---- (1) the guard pass against a plain fp32 sum of the same bytes
    g = torch.randn(n, device=dev)
    store = type("S", (), {"g32": g, "dev": dev})()
    guard = GradGuard(max_grad_norm=1.0, skip_nonfinite=True)
    res = alternate({"torch f32 sum read": lambda: g.sum(), "uniir_grad_guard + finish": lambda: guard.measure([(store, 0, n)], 1.0)},
                    a.reps)
    print("(1) norm / scan pass")
    t_sum = line("torch f32 sum read", res["torch f32 sum read"], 4 * n)
    t_guard = line("uniir_grad_guard + finish", res["uniir_grad_guard + finish"], 4 * n)
    print(f"  ratio guard / sum read: {t_guard / t_sum:.3f} (expected <= 1.15)")
    guard.publish()
    guard.resolve()
    ref = float(g.double().square().sum().sqrt())
    print(f"  norm {guard.stats['norm']!r}  torch f64 {ref!r}  rel diff {abs(guard.stats['norm'] - ref) / ref:.2e}")

    # ---- (2) guarded against plain AdamW, same buffers
    p, m, v = torch.randn(n, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev)
    w16 = torch.empty(n, device=dev, dtype=torch.bfloat16)
    g.mul_(1e-3)
    guard.measure([(store, 0, n)], 1.0)          # a control block with skip 0 (coef below 1: the multiply is live)
    args = (p, g, m, v, w16, n, 1e-5, 0.9, 0.98, 1e-6, 0.2, 1, 1.0)
    res = alternate({"uniir_adamw_step": lambda: ops.call("uniir_adamw_step", *args),
                     "uniir_adamw_step_guarded": lambda: ops.call("uniir_adamw_step_guarded", *args, guard.ctl)}, a.reps)
    print("(2) AdamW over the same buffers (22 B / parameter)")
    t_plain = line("uniir_adamw_step", res["uniir_adamw_step"], 22 * n)
    t_guarded = line("uniir_adamw_step_guarded", res["uniir_adamw_step_guarded"], 22 * n)
    spread = max(res["uniir_adamw_step"]) - min(res["uniir_adamw_step"])
    print(f"  guarded - plain: {t_guarded - t_plain:+.1f} us; spread (max - min) of the plain kernel's own runs: {spread:.1f} us")
    del p, m, v, w16, g, store

    # ---- (3) a whole train step
    if a.step:
        import time
        from types import SimpleNamespace
        from bench import synth_batch
        from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
        from uniir_amd.clip_model import CLIP_CONFIGS
        from uniir_amd.trainer import NativeTrainer
        torch.cuda.empty_cache()
        config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=True), data_config=SimpleNamespace(in_batch_neg_num=0))
        model = CLIPScoreFusion("ViT-L/14", device=dev, config=config)
        tr = NativeTrainer(model, t_total=1000)
        batch = synth_batch(CLIP_CONFIGS["ViT-L/14"], a.pairs, 2023, dev)
        on = GradGuard(max_grad_norm=1e30, skip_nonfinite=True)          # measures and decides, changes no step

        def step(g_):
            tr.opt.guard = g_
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = tr.train_step(batch)
            out["loss"].item()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        for _ in range(3):
            step(None), step(on)
        ts = {"off": [], "on": []}
        for _ in range(10):
            ts["off"].append(step(None))
            ts["on"].append(step(on))
        print(f"(3) CLIP_SF ViT-L/14 train step at {a.pairs} pairs, ms")
        for k, t in ts.items():
            print(f"  guard {k:<4s} median {statistics.median(t):8.2f}  min {min(t):8.2f}  max {max(t):8.2f}")
        print(f"  on - off (medians): {statistics.median(ts['on']) - statistics.median(ts['off']):+.2f} ms; "
              f"last step's stats {tr.opt.grad_stats()}")


if __name__ == "__main__":
    main()
