"""Embedding rate of CLIP_FF in bf16 and in fp16 (CLIPFeatureFusion.encode_multimodal_input with precision "bf16" / "fp16": the towers
without pooling -> 2-layer T5 stack with the relative bias -> mean pool) at the real architectures, random weights, images and tokens
(dev tool).  The two precisions alternate in one process on one box, RUNS runs each of ITERS timed forwards after one warm-up of each
precision at the timed shape (device events around every forward, the median of a run), with the board's shader clock and power beside
every run (bench.BoardSampler: the amdgpu hwmon files, best effort).
Before the rates: the relative L2 distance of each precision from oracle/clipff_oracle.py (fp32, CPU) on the tiny model with the token
geometry of ViT-L/14@336px (654 fused tokens), and with --kernels the time per launch of uniir_attn_rel_fwd_f16 against
uniir_attn_rel_fwd_long_f16 and their bf16 twins at 334 and 512 tokens (256 items x 12 heads, device events, 20 launches after 3).
    python tools/clipff_embed_rate.py [--models ViT-B/32,ViT-L/14,ViT-L/14@336px] [--items 256] [--iters 5] [--runs 2] [--kernels] [--out FILE]
--mode bf16 | fp16 runs one precision only (ITERS forwards, no oracle): the program to put behind `rocprofv3 --kernel-trace --stats --`."""
import argparse
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))
import torch  # noqa: E402


def _sampler():
    try:
        import bench
        return bench.BoardSampler(0)
    except Exception:
        return None


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
    """each precision against the fp32 oracle on the tiny model of 654 fused tokens (2 + 2 tower layers of width 128, T5 d_model 128, 2
    heads, 2 layers; 4 items), with the q projections scaled by d_kv^-0.5 and as the module draws them"""
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from oracle import clip_oracle as O
    from oracle import clipff_oracle as FF
    from uniir_amd import clip_model
    t5_cfg = dict(d_model=128, num_heads=2, d_ff=256, num_layers=2, d_kv=64)
    cfg = O.tiny_config(image_resolution=336, vision_patch_size=14, vision_width=128, vision_layers=2, transformer_width=128,
                        transformer_heads=2, embed_dim=128)
    clip_model.CLIP_CONFIGS["tiny-ff-336-rate"] = cfg
    batch = O.synthetic_batch(cfg, 2, seed=23)
    for gain, what in ((t5_cfg["d_kv"] ** -0.5, "q scaled by d_kv^-0.5"), (1.0, "q as the module draws it")):
        m = CLIPFeatureFusion("tiny-ff-336-rate", device="cuda", t5_config={k: v for k, v in t5_cfg.items() if k != "d_kv"} | {"dropout_rate": 0.0})
        sd = O.init_state_dict(cfg, seed=5)
        sd.pop("text_projection")
        m.clip_model.load_state_dict(sd, strict=True)
        with torch.no_grad():
            for n, p in m.t5_layers.named_parameters():
                if n.endswith("SelfAttention.q.weight"):
                    p.mul_(gain)
            t5 = {n: p.detach().cpu().clone() for n, p in m.t5_layers.named_parameters()}
            want = FF.encode_multimodal_input(sd, t5, cfg, t5_cfg, batch["txt_batched"], batch["image_batched"]).double()
        m.eval()
        d = {p: float((_encode(m, p, batch["txt_batched"].cuda(), batch["image_batched"].cuda()).double().cpu() - want).norm() / want.norm())
             for p in ("bf16", "fp16")}
        say(f"relative L2 distance from the fp32 oracle (tiny CLIP_FF, 654 fused tokens, 4 items, {what}): bf16 {d['bf16']:.3e}  "
            f"fp16 {d['fp16']:.3e}  ratio {d['fp16'] / d['bf16']:.3f}")


def _timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def kernels(say, items=256, heads=12, passes=2):
    """time per launch of the four forward entry points of the relative-bias attention at the sizes both forms take"""
    from uniir_amd import ops
    from uniir_amd.clipff_model import T5_BUCKETS, rel_bucket_table
    W = heads * 64
    for ps in range(passes):
        for T in (334, 512):
            g = torch.Generator().manual_seed(T)
            x = torch.randn(items * T, 3 * W, generator=g).cuda()
            x[:, :W] *= 0.125          # T5 applies no 1 / sqrt(d): its q is small instead
            emb, table = torch.randn(T5_BUCKETS, heads, generator=g).cuda(), rel_bucket_table(T).cuda()
            lse = torch.empty(items, heads, T, device="cuda")
            line = []
            for dt, names in ((torch.bfloat16, ("uniir_attention_rel_fwd", "uniir_attention_rel_fwd_long")),
                              (torch.float16, ("uniir_attn_rel_fwd_f16", "uniir_attn_rel_fwd_long_f16"))):
                qkv, out = x.to(dt), torch.empty(items * T, W, device="cuda", dtype=dt)
                for name in names:
                    tail = (0.0, 0) if dt == torch.bfloat16 else ()
                    ms = _timeit(lambda: ops.call(name, qkv, out, lse, emb, table, T5_BUCKETS, 1.0, items, T, heads, *tail))
                    line.append(f"{name} {ms:.3f} ms")
            say(f"pass {ps + 1} rel attn forward {T} tokens, {items} items x {heads} heads: " + " | ".join(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="ViT-B/32,ViT-L/14,ViT-L/14@336px")
    ap.add_argument("--items", type=int, default=256)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--mode", default="both", choices=("both", "bf16", "fp16"))
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clipff_embed_rate.py measures on the GPU; there is none here")
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from uniir_amd.clip_model import CLIP_CONFIGS
    out = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}")
    if a.mode == "both":
        distances(say)
    if a.kernels:
        kernels(say)
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    for name in [n for n in a.models.split(",") if n]:
        model = CLIPFeatureFusion(name, device="cuda", config=config).eval()
        cfg = CLIP_CONFIGS[name]
        px = cfg["image_resolution"]
        g = torch.Generator(device="cuda").manual_seed(px)
        images = torch.randn(a.items, 3, px, px, device="cuda", generator=g)
        txt = torch.randint(1, cfg["vocab_size"] - 2, (a.items, cfg["context_length"]), device="cuda", generator=g)
        txt[:, -1] = cfg["vocab_size"] - 1
        tokens = cfg["context_length"] + (px // cfg["vision_patch_size"]) ** 2 + 1
        precisions = ("bf16", "fp16") if a.mode == "both" else (a.mode,)
        warm = {p: _encode(model, p, txt, images).float() for p in precisions}          # warm-up of every timed shape, and the check
        torch.cuda.synchronize()
        note = ""
        if a.mode == "both":
            note = f"; relative L2 difference of the bf16 and fp16 embeddings {((warm['bf16'] - warm['fp16']).norm() / warm['fp16'].norm()).item():.2e}"
        del warm
        say(f"CLIP_FF {name}, {a.items} items of {px} pixels ({tokens} fused tokens), {a.iters} forwards per run{note}")
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
