"""Forward rate of the BLIP vision encoder in bf16 and in fp16 (BLIPFeatureFusion._vit_tokens, the per-op ViT of blip_model.vit_forward)
at the real architecture, random weights and images (dev tool).  The two precisions alternate on one box, RUNS runs each of ITERS
timed forwards after one warm-up of each shape (device events around every forward, the median of a run), with the board's shader clock
and power beside every run (bench.BoardSampler: the amdgpu hwmon files, best effort).  Also the largest difference between the two
token sets, as a check that both computed the same thing.
    python tools/blip_vit_rate.py [--vit large] [--pixels 224,384] [--items 1024] [--iters 5] [--runs 2]"""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from uniir_amd.blip_model import BLIPFeatureFusion

MED_SMALL = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=1, vocab_size=64,
                 max_position_embeddings=32)          # the text side is not run: kept small


def _sampler():
    try:
        import bench
        return bench.BoardSampler(0)
    except Exception:
        return None


def _run(model, images, precision, iters):
    s = _sampler()
    if s is not None:
        s.start()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        model._vit_tokens(images, precision)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    board = s.stop() if s is not None else None
    ts.sort()
    return ts[len(ts) // 2], board


def vit_flops(cfg, tokens):
    """multiply-adds x 2 of one item's forward: the patch embedding, per block the four projections and the two attention products"""
    D, P, depth = cfg["embed_dim"], cfg["patch_size"], cfg["depth"]
    per_block = 2 * tokens * (3 * D * D + D * D + 8 * D * D) + 4 * tokens * tokens * D
    return 2 * (tokens - 1) * 3 * P * P * D + depth * per_block


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vit", default="large")
    ap.add_argument("--pixels", default="224,384")
    ap.add_argument("--items", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blip_vit_rate.py measures on the GPU; there is none here")
    for px in (int(x) for x in a.pixels.split(",")):
        model = BLIPFeatureFusion(med_config=MED_SMALL, image_size=px, vit=a.vit, embed_dim=MED_SMALL["hidden_size"], queue_size=16,
                                  config=types.SimpleNamespace(tokenizer_max_length=20), seed=1).cuda().eval()
        g = torch.Generator(device="cuda").manual_seed(px)
        images = torch.randn(a.items, 3, px, px, device="cuda", generator=g)
        tokens = (px // model.vit_cfg["patch_size"]) ** 2 + 1
        tb = model._vit_tokens(images, "bf16").float()          # warm-up of both, and the check
        th = model._vit_tokens(images, "fp16").float()
        torch.cuda.synchronize()
        diff = ((tb - th).norm() / th.norm()).item()
        del tb, th
        print(f"BLIP ViT-{a.vit} forward, {a.items} images of {px} pixels ({tokens} tokens), {a.iters} forwards per run; "
              f"relative L2 difference of the bf16 and fp16 tokens {diff:.2e}")
        fl = vit_flops(model.vit_cfg, tokens) * a.items
        res = {"bf16": [], "fp16": []}
        for r in range(a.runs):
            for prec in ("bf16", "fp16"):
                ms, board = _run(model, images, prec, a.iters)
                res[prec].append(ms)
                b = "board not sampled" if not board else f"{board['sclk_mhz_mean']:.0f} MHz, {board['power_w_mean']} W"
                print(f"  run {r} {prec}: {ms:8.2f} ms  {a.items / ms * 1e3:8.1f} images/s  {fl / ms / 1e9:7.1f} TFLOP/s executed  ({b})")
        mb, mh = min(res["bf16"]), min(res["fp16"])
        sp = max(max(v) - min(v) for v in res.values())
        print(f"  fp16 / bf16 time {mh / mb:.3f} (best run of each); spread between the runs of one precision up to {sp:.2f} ms")
        del model, images
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
