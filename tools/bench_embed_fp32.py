"""Forward-only embedding rate at precision "fp32" beside "bf16" for BLIP_FF (base, large) and CLIP_FF (ViT-B/32, ViT-L/14@336px) at the
real architectures with random weights, images and tokens, and the time the fp32 attention kernels (uniir_attention_f32_fwd,
uniir_attn_f32_rel_fwd) take inside one fp32 forward (dev tool; no rate is a target, the output is the record).
Per model: one warm-up of each precision at the timed shape, then RUNS runs of ITERS forwards each, precisions alternating, device
events around every forward, the median of a run; the board's shader clock and power beside every run (bench.BoardSampler, best
effort).  The attention share: one more fp32 forward with a device-event pair around every call of the two entry points.
    python tools/bench_embed_fp32.py [--models blip_base,blip_large,ViT-B/32,ViT-L/14@336px] [--items 32] [--iters 3] [--runs 2]
                                     [--image-size 224] [--out profiles/embed_fp32.txt]"""
import argparse
import os
import socket
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))
import torch  # noqa: E402

ATTENTION_F32 = ("uniir_attention_f32_fwd", "uniir_attn_f32_rel_fwd")


def _sampler():
    try:
        import bench
        return bench.BoardSampler(0)
    except Exception:
        return None


def _run(encode, precision, iters):
    s = _sampler()
    if s is not None:
        s.start()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        encode(precision)
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    board = s.stop() if s is not None else None
    ts.sort()
    return ts[len(ts) // 2], board


def attention_share(encode):
    """-> (ms of the whole fp32 forward, ms inside the fp32 attention entry points, their calls) of one forward"""
    from uniir_amd import _lib
    lib = _lib.load()
    pairs, real = [], {n: getattr(lib, n) for n in ATTENTION_F32}

    def timed(name):
        def f(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = real[name](*a)
            e1.record()
            pairs.append((e0, e1))
            return rc
        return f

    for n in ATTENTION_F32:
        setattr(lib, n, timed(n))
    try:
        w0, w1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        w0.record()
        encode("fp32")
        w1.record()
        torch.cuda.synchronize()
    finally:
        for n in ATTENTION_F32:
            setattr(lib, n, real[n])
    return w0.elapsed_time(w1), sum(a.elapsed_time(b) for a, b in pairs), len(pairs)


def build(name, items, image_size):
    """-> (label, encode(precision)) of one model on random inputs"""
    if name.startswith("blip_"):
        from uniir_amd import blip_model as bm
        L = 40
        model = bm.BLIPFeatureFusion(med_config={}, image_size=image_size, vit=name[5:], queue_size=16,
                                     config=SimpleNamespace(tokenizer_max_length=L)).cuda().eval()
        g = torch.Generator(device="cuda").manual_seed(image_size)
        images = torch.randn(items, 3, image_size, image_size, device="cuda", generator=g)
        ids = torch.randint(3, 30000, (items, L), device="cuda", generator=g)
        lens = torch.randint(5, L + 1, (items,), device="cuda", generator=g)
        mask = (torch.arange(L, device="cuda")[None, :] < lens[:, None]).long()
        txt = SimpleNamespace(input_ids=ids * mask, attention_mask=mask)
        tokens = (image_size // model.vit_cfg["patch_size"]) ** 2 + 1
        label = f"BLIP_FF {name[5:]}, {items} items of {image_size} pixels ({tokens} image tokens, {L} text positions)"
    else:
        from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
        from uniir_amd.clip_model import CLIP_CONFIGS
        config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
        model = CLIPFeatureFusion(name, device="cuda", config=config).eval()
        cfg = CLIP_CONFIGS[name]
        px = cfg["image_resolution"]
        g = torch.Generator(device="cuda").manual_seed(px)
        images = torch.randn(items, 3, px, px, device="cuda", generator=g)
        txt = torch.randint(1, cfg["vocab_size"] - 2, (items, cfg["context_length"]), device="cuda", generator=g)
        txt[:, -1] = cfg["vocab_size"] - 1
        tokens = cfg["context_length"] + (px // cfg["vision_patch_size"]) ** 2 + 1
        label = f"CLIP_FF {name}, {items} items of {px} pixels ({tokens} fused tokens)"

    model.embed_fp32 = True          # the opt-in that makes "fp32" a precision the module knows

    def encode(precision):
        model.precision = precision
        try:
            with torch.no_grad():
                return model.encode_multimodal_input(txt, images)
        finally:
            model.precision = "bf16"

    return label, encode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="blip_base,blip_large,ViT-B/32,ViT-L/14@336px")
    ap.add_argument("--items", type=int, default=32)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--image-size", type=int, default=224, help="BLIP's image size (384: 577 image tokens)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_embed_fp32.py measures on the GPU; there is none here")
    out = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}  box: {socket.gethostname()}  clock: {time.strftime('%Y-%m-%d %H:%M:%S %Z')}")
    for name in [n for n in a.models.split(",") if n]:
        label, encode = build(name, a.items, a.image_size)
        warm = {p: encode(p).float() for p in ("bf16", "fp32")}          # warm-up of both timed shapes, and the check
        torch.cuda.synchronize()
        d = ((warm["bf16"] - warm["fp32"]).norm() / warm["fp32"].norm()).item()
        del warm
        say(f"{label}, {a.iters} forwards per run; relative L2 difference of the bf16 and fp32 embeddings {d:.2e}")
        best = {}
        for r in range(a.runs):
            for prec in ("bf16", "fp32"):
                ms, board = _run(encode, prec, a.iters)
                best[prec] = min(best.get(prec, ms), ms)
                b = "board not sampled" if not board else f"{board['sclk_mhz_mean']:.0f} MHz, {board['power_w_mean']} W"
                say(f"  run {r} {prec}: {ms:9.2f} ms  {a.items / ms * 1e3:8.1f} items/s  ({b})")
        whole, att, calls = attention_share(encode)
        say(f"  fp32 / bf16 time {best['fp32'] / best['bf16']:.1f} (best run of each); fp32 attention kernels: {att:.2f} ms of a "
            f"{whole:.2f} ms fp32 forward in {calls} calls = {100 * att / whole:.1f} %")
        del encode
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
