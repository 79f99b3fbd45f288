"""Embedding rate of BLIP_FF in bf16 and in fp16 (BLIPFeatureFusion.encode_multimodal_input with precision "bf16" / "fp16": ViT -> MED
BERT with cross-attention -> pooler) at the real architectures, random weights, images and captions (dev tool).  The two precisions
alternate in one process on one box, RUNS runs each of ITERS timed forwards after one warm-up of each precision at the timed shape
(device events around every forward, the median of a run), with the board's shader clock and power beside every run
(bench.BoardSampler: the amdgpu hwmon files, best effort).  Captions are 100 positions with valid lengths U{5..100}, as in bench.py;
pack_text is on, pool_last_layer as the environment sets it.
Before the rates: the relative L2 distance of each precision from oracle/blip_oracle.py (fp32, CPU) at one small geometry.
    python tools/blip_embed_rate.py [--vit base,large] [--pixels 224,384] [--items 256] [--iters 5] [--runs 2] [--out FILE]
--mode bf16 | fp16 runs one precision only (ITERS forwards, no oracle): the program to put behind `rocprofv3 --kernel-trace --stats --`."""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from uniir_amd.blip_model import MED_DEFAULT, BLIPFeatureFusion

L = 100
MED_SMALL = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=2, vocab_size=64,
                 max_position_embeddings=128)
VIT_SMALL = dict(img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2, drop_path_rate=0.0)


def _sampler():
    try:
        import bench
        return bench.BoardSampler(0)
    except Exception:
        return None


def _captions(items, vocab, length, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (items, length), generator=g)
    ids[:, 0] = 1
    lens = torch.randint(5, length + 1, (items,), generator=g) if length >= 5 else torch.full((items,), length)
    mask = (torch.arange(length).unsqueeze(0) < lens.unsqueeze(1)).long()
    return ids * mask, mask


def _encode(model, precision, txt, images):
    model.precision = precision
    try:
        with torch.no_grad():
            return model.encode_multimodal_input(txt, images)
    finally:
        model.precision = "bf16"


def _run(model, txt, images, precision, iters):
    s = _sampler()
    if s is not None:
        s.start()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _encode(model, precision, txt, images)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    board = s.stop() if s is not None else None
    ts.sort()
    return ts[len(ts) // 2], board


def distances(say):
    """each precision against the fp32 oracle at one small geometry (64 pixels, 17 image tokens, 2 + 2 layers, 8 captions of 20)"""
    from oracle import blip_oracle as bo
    model = BLIPFeatureFusion(med_config=MED_SMALL, vit_config=VIT_SMALL, embed_dim=MED_SMALL["hidden_size"], queue_size=16,
                              config=types.SimpleNamespace(tokenizer_max_length=20), seed=2).cuda().eval()
    ids, mask = _captions(8, MED_SMALL["vocab_size"], 20, 3)
    img = torch.randn(8, 3, 64, 64, generator=torch.Generator().manual_seed(4))
    sd = {n: p.detach().cpu().float() for n, p in model.named_parameters()}
    with torch.no_grad():
        want = bo.encode_multimodal_input(sd, ids, mask, img, model.vit_cfg, model.med_cfg).double()
    txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    d = {p: float((_encode(model, p, txt, img.cuda()).double().cpu() - want).norm() / want.norm()) for p in ("bf16", "fp16")}
    say(f"relative L2 distance from the fp32 oracle (tiny BLIP_FF, 8 items): bf16 {d['bf16']:.3e}  fp16 {d['fp16']:.3e}  "
        f"ratio {d['fp16'] / d['bf16']:.3f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--vit", default="base,large")
    ap.add_argument("--pixels", default="224,384")
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--mode", default="both", choices=("both", "bf16", "fp16"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("blip_embed_rate.py measures on the GPU; there is none here")
    out = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}")
    if a.mode == "both":
        distances(say)
    for vit in a.vit.split(","):
        for px in (int(x) for x in a.pixels.split(",")):
            model = BLIPFeatureFusion(med_config=dict(MED_DEFAULT), image_size=px, vit=vit, embed_dim=MED_DEFAULT["hidden_size"], queue_size=16,
                                      config=types.SimpleNamespace(tokenizer_max_length=L), seed=1).cuda().eval()
            g = torch.Generator(device="cuda").manual_seed(px)
            images = torch.randn(a.items, 3, px, px, device="cuda", generator=g)
            ids, mask = _captions(a.items, MED_DEFAULT["vocab_size"], L, px)
            txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
            tokens = (px // model.vit_cfg["patch_size"]) ** 2 + 1
            precisions = ("bf16", "fp16") if a.mode == "both" else (a.mode,)
            warm = {p: _encode(model, p, txt, images).float() for p in precisions}          # warm-up of every timed shape, and the check
            torch.cuda.synchronize()
            note = ""
            if a.mode == "both":
                note = f"; relative L2 difference of the bf16 and fp16 embeddings {((warm['bf16'] - warm['fp16']).norm() / warm['fp16'].norm()).item():.2e}"
            rows = model.last_text_rows
            del warm
            say(f"BLIP_FF ViT-{vit} + BERT-base, {a.items} items of {px} pixels ({tokens} image tokens), captions of {L} with "
                f"{rows[0]} of {rows[1]} rows live, pool_last_layer {model.pool_last_layer}, {a.iters} forwards per run{note}")
            res = {p: [] for p in precisions}
            for r in range(a.runs):
                for prec in precisions:
                    ms, board = _run(model, txt, images, prec, a.iters)
                    res[prec].append(ms)
                    b = "board not sampled" if not board else f"{board['sclk_mhz_mean']:.0f} MHz, {board['power_w_mean']} W"
                    say(f"  run {r} {prec}: {ms:8.2f} ms  {a.items / ms * 1e3:8.1f} items/s  ({b})")
            if a.mode == "both":
                mb, mh = min(res["bf16"]), min(res["fp16"])
                sp = max(max(v) - min(v) for v in res.values())
                say(f"  fp16 / bf16 time {mh / mb:.3f} (best run of each): fp16 rate {100 * (mb / mh - 1):+.1f} % of bf16's; spread between "
                    f"the runs of one precision up to {sp:.2f} ms")
            del model, images, txt
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
