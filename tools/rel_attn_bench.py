"""Time per launch of the T5 relative-bias self-attention of the CLIP_FF fusion stack (dev tool; device events, 20 timed launches
after 3): uniir_attention_rel_fwd / _rel_bwd (the resident kernels, seq <= 512) or uniir_attention_rel_fwd_long / _rel_bwd_long (the
streaming kernels, seq <= 1024) at 256 items x 12 heads, scale 1, 32 buckets, dropout 0 and 0.1; the backward includes the drel
reduction into a [32][12] table.  654 tokens are CLIP_FF at ViT-L/14@336px (77 + 577), 334 at ViT-L/14.
The comparison with the parent build, as recorded in profiles/attention_rel_long.txt: export the parent commit's uniir_amd/ and
include/ into a directory of its own (git archive <parent> uniir_amd include | tar -x -C DIR), make -C DIR/uniir_amd/csrc, copy this
file to DIR/tools/ and run that copy with RA_SEQ=512 RA_FORM=resident (the tool imports the uniir_amd package next to it),
alternating with this tree's copy at RA_SEQ=654 in one session.  The expectation (the step from resident to
streamed operands, scaled to a square call): time at 654 tokens <= 1.5 x (21 / 16)^2 x the parent's time at 512 tokens.
  RA_SEQ ("654")  RA_FORM (long | resident; default: long above 512 tokens)  RA_ITEMS (256)  RA_HEADS (12)  RA_PASSES (2)
  RA_TAG (printed in front of every line)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from uniir_amd import ops  # noqa: E402
from uniir_amd.clipff_model import T5_BUCKETS, rel_bucket_table  # noqa: E402

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


def one(tag, b, H, T, form, p):
    W = H * 64
    sfx = "_long" if form == "long" else ""
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(b * T, 3 * W, generator=g).to(dev)
    qkv[:, :W] *= 0.125          # T5 applies no 1 / sqrt(d): its q is small instead
    qkv = qkv.bfloat16()
    emb = torch.randn(T5_BUCKETS, H, generator=g).to(dev)
    table = rel_bucket_table(T).to(dev)
    out = torch.empty(b * T, W, device=dev, dtype=torch.bfloat16)
    lse = torch.empty(b, H, T, device=dev)
    fwd = lambda: ops.call("uniir_attention_rel_fwd" + sfx, qkv, out, lse, emb, table, T5_BUCKETS, 1.0, b, T, H, p, 7)          # noqa: E731
    fwd()
    do = torch.randn(b * T, W, generator=g).to(dev).bfloat16()
    dqkv = torch.empty_like(qkv)
    drel = torch.zeros(T5_BUCKETS, H, device=dev)
    bwd = lambda: ops.call("uniir_attention_rel_bwd" + sfx, qkv, out, do, lse, dqkv, emb, table, T5_BUCKETS, 1.0, drel, b, T, H, p, 7)          # noqa: E731
    bwd()
    torch.cuda.synchronize()
    chk = f"out {out.float().abs().sum().item():.1f} dqkv {dqkv.float().abs().sum().item():.1f} drel {drel.abs().sum().item():.3f}"
    tf, tb = timeit(fwd), timeit(bwd)
    print(f"{tag} rel attn {T:4d} tokens b={b} H={H} {form:8s} drop={p:.1f}: fwd {tf:.3f} ms | bwd {tb:.3f} ms  chk {chk}", flush=True)


def main():
    b, H = int(os.environ.get("RA_ITEMS", "256")), int(os.environ.get("RA_HEADS", "12"))
    tag = os.environ.get("RA_TAG", "")
    for ps in range(int(os.environ.get("RA_PASSES", "2"))):
        for T in (int(x) for x in os.environ.get("RA_SEQ", "654").split(",")):
            form = os.environ.get("RA_FORM") or ("long" if T > 512 else "resident")
            for p in (0.0, 0.1):
                one(f"{tag} pass {ps + 1}", b, H, T, form, p)


if __name__ == "__main__":
    main()
