"""Timing of the kernels whose sums became order-fixed (dev tool; profiles/reproducible_all.txt): uniir_attention_rel_bwd at CLIP_FF's
shape, uniir_text_embed_bwd dense and packed at 1024 captions.  It uses only entry points that the parent commit has too, so one
file times both trees:   python tools/reproducible_ab.py [--items 512 --heads 16 --seq 334]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from uniir_amd import clipff_model, ops

dev = "cuda"


def timeit(fn, iters=20, warm=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=512)          # CLIP_FF at 256 pairs: 512 fused sequences
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--seq", type=int, default=334)
    a = ap.parse_args()
    torch.manual_seed(0)
    b, H, T, nb = a.items, a.heads, a.seq, clipff_model.T5_BUCKETS
    W = H * 64
    qkv = (torch.randn(b * T, 3 * W, device=dev) * 0.35).bfloat16()
    emb = torch.randn(nb, H, device=dev)
    table = clipff_model.rel_bucket_table(T).to(dev)
    out, lse = torch.empty(b * T, W, device=dev, dtype=torch.bfloat16), torch.empty(b, H, T, device=dev)
    for p in (0.0, 0.1):
        ops.call("uniir_attention_rel_fwd", qkv, out, lse, emb, table, nb, 1.0, b, T, H, p, 77)
        do, dqkv, drel = torch.randn_like(out), torch.empty_like(qkv), torch.zeros(nb, H, device=dev)
        ms = timeit(lambda: ops.call("uniir_attention_rel_bwd", qkv, out, do, lse, dqkv, emb, table, nb, 1.0, drel, b, T, H, p, 77))
        print(f"attention_rel_bwd items={b} heads={H} seq={T} drop={p}: {ms:.3f} ms")
    n, ctx, w, vocab = 1024, 77, 768, 49408
    ids = torch.randint(1000, 40000, (n, ctx), dtype=torch.int32)
    lens = torch.randint(8, ctx + 1, (n,))
    ids[:, 0] = 49406
    ids[torch.arange(n), lens - 1] = 49407
    ids = torch.where(torch.arange(ctx).unsqueeze(0) < lens.unsqueeze(1), ids, torch.zeros_like(ids)).to(dev)      # id 0 behind the EOT
    live = (torch.arange(ctx).unsqueeze(0) < lens.unsqueeze(1)).flatten().to(dev)
    dx = torch.randn(n * ctx, w, device=dev) * live.unsqueeze(1)
    dt, dp = torch.zeros(vocab, w, device=dev), torch.zeros(ctx, w, device=dev)
    ms = timeit(lambda: ops.call("uniir_text_embed_bwd", ids, dx, dt, dp, n, ctx, w, vocab))
    print(f"text_embed_bwd dense {n} x {ctx} x {w} ({int((~live).sum())} rows of the padding id): {ms:.3f} ms")
    row_off = torch.zeros(n + 1, dtype=torch.int32)
    row_off[1:] = torch.cumsum(lens, 0)
    ro, dxp = row_off.to(dev), dx[live].contiguous()
    ms = timeit(lambda: ops.call("uniir_text_embed_bwd_packed", ids, dxp, ro, dt, dp, n, ctx, w, vocab))
    print(f"text_embed_bwd packed {n} x {ctx} x {w} ({int(live.sum())} rows): {ms:.3f} ms")
    if hasattr(ops, "reduce_stats"):
        print("reduce_stats (fallbacks, max_request):", ops.reduce_stats())


if __name__ == "__main__":
    main()
