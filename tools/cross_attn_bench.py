"""Time per launch of BLIP's MED cross-attention (dev tool; device events): ops.attention_fwd_ex / attention_bwd_ex at 256 items x 12
heads, tq text queries against tk image keys, dense and with packed query rows (lengths uniform in 5 .. tq), dropout 0 and 0.1.
tk = 577 (a 384-pixel ViT) runs uniir_attention_fwd_long / _bwd_long; tk <= 512 the resident kernels, which is also what a build from
before those entry points can run: XA_TK=512 with that build's tree is the comparison line of profiles/attention_cross_long.txt.
The comparison with the parent build, as recorded there: export the parent commit's uniir_amd/ and include/ into a directory of its own
(git archive <parent> uniir_amd include | tar -x -C DIR), make -C DIR/uniir_amd/csrc, copy this file to DIR/tools/ and run that copy
with XA_TK=512 (the tool imports the uniir_amd package next to it), alternating with this tree's copy at XA_TK=577 in one session.
  XA_TK (577)  XA_TQ ("35,100")  XA_ITEMS (256)  XA_HEADS (12)  XA_PASSES (2)  XA_TAG (printed in front of every line)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from uniir_amd import ops  # noqa: E402

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


def one(tag, b, H, tq, tk, packed, p):
    W = H * 64
    g = torch.Generator().manual_seed(tq * 1000 + tk)
    if packed:
        lens = torch.randint(5, tq + 1, (b,), generator=g)
        off = torch.zeros(b + 1, dtype=torch.int32)
        off[1:] = lens.cumsum(0)
        rows = int(off[-1])
        kw = dict(row_off=off.to(dev), kv_packed=False)
    else:
        rows, kw = b * tq, {}
    q = torch.randn(rows, W, device=dev).bfloat16()
    kv = torch.randn(b * tk, 2 * W, device=dev).bfloat16()
    fkw = dict(kw, rows=rows) if packed else kw
    fwd = lambda: ops.attention_fwd_ex(q, W, kv, kv[:, W:], 2 * W, b, tq, tk, H, drop_p=p, drop_seed=7, **fkw)          # noqa: E731
    out, lse = fwd()
    do = torch.randn_like(out)
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    bwd = lambda: ops.attention_bwd_ex(q, W, kv, kv[:, W:], 2 * W, out, do, lse, dq, W, dkv, dkv[:, W:], 2 * W, b, tq, tk, H,          # noqa: E731
                                       drop_p=p, drop_seed=7, **kw)
    tf, tb = timeit(fwd), timeit(bwd)
    print(f"{tag} cross attn {tq:4d} x {tk} b={b} H={H} {'packed' if packed else 'dense '} rows={rows:6d} drop={p:.1f}: fwd {tf:.3f} ms | "
          f"bwd {tb:.3f} ms  chk out {out.float().abs().sum().item():.1f} dq {dq.float().abs().sum().item():.1f} "
          f"dkv {dkv.float().abs().sum().item():.1f}", flush=True)


def main():
    tk = int(os.environ.get("XA_TK", "577"))
    b, H = int(os.environ.get("XA_ITEMS", "256")), int(os.environ.get("XA_HEADS", "12"))
    tag = os.environ.get("XA_TAG", "")
    for ps in range(int(os.environ.get("XA_PASSES", "2"))):
        for tq in (int(x) for x in os.environ.get("XA_TQ", "35,100").split(",")):
            for packed in (False, True):
                for p in (0.0, 0.1):
                    one(f"{tag} pass {ps + 1}", b, H, tq, tk, packed, p)


if __name__ == "__main__":
    main()
