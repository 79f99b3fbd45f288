"""Microbenchmark of uniir_gemm_wgrad_ln_bwd at the ViT-L/14 x 1024-image shapes: each fused pair (a weight gradient with the
LayerNorm backward in its launch) against the two launches it replaces, in one process, interleaved, median of REPS rounds.

    python tools/wgrad_ln_pair_ab.py [rows=263168]

Pairs: dW_fc (4096 x 1024, 64 tiles) with ln_2's backward, dW_qkv (3072 x 1024, 48 tiles, + bias row sums) with ln_1's, for every
count of side compute units that has a chunk plan.  Times are HIP-event times around the whole call (main launch + the partial and
slab reductions)."""
import ctypes as C
import statistics
import sys

import torch

sys.path.insert(0, __file__.rsplit("/tools/", 1)[0])
from uniir_amd import _lib, ops  # noqa: E402

REPS = 7
DEV = "cuda"
BF16 = torch.bfloat16


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 263168
    W = 1024
    lib, st = _lib.load(), ops._stream()
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.randn(rows, W, device=DEV, generator=g)
    dy = torch.randn(rows, W, device=DEV, generator=g).to(BF16)
    dres = torch.randn(rows, W, device=DEV, generator=g)
    gamma = torch.ones(W, device=DEV)
    dx, dxb = torch.empty(rows, W, device=DEV), torch.empty(rows, W, device=DEV, dtype=BF16)
    dg, db, cs = (torch.zeros(W, device=DEV) for _ in range(3))
    ws = torch.empty(16 * 4096 * 1024 * 4, dtype=torch.uint8, device=DEV)
    ln = (x.data_ptr(), W, gamma.data_ptr(), dy.data_ptr(), 0, dres.data_ptr(), dx.data_ptr(), W, dxb.data_ptr(), dg.data_ptr(),
          db.data_ptr(), cs.data_ptr(), None, rows, W, 1e-5)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for name, M, bias in (("dW_fc + ln_2", 4096, False), ("dW_qkv + ln_1", 3072, True)):
        A = torch.randn(rows, M, device=DEV, generator=g).to(BF16)
        B = torch.randn(rows, W, device=DEV, generator=g).to(BF16)
        dW = torch.zeros(M, W, device=DEV)
        rs = torch.zeros(M, device=DEV)
        tiles = (M // 256) * (W // 256)
        d = _lib.GemmDesc()
        d.A, d.B, d.C = A.data_ptr(), B.data_ptr(), dW.data_ptr()
        d.M, d.N, d.K, d.lda, d.ldb, d.ldc = M, W, rows, M, W, W
        d.a_tmaj = d.b_tmaj = 1
        d.epilogue, d.dtype, d.alpha = 5, 0, 1.0
        d.k_splits = lib.uniir_gemm_wgrad_splits(rows, tiles)
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel()
        d.a_rowsum = rs.data_ptr() if bias else None
        sides = [c for c in (16, 24, 32, 40, 48, 56, 64, 96) if 0 < lib.uniir_gemm_wgrad_side_plan(rows, tiles, c) * M * W * 4 <= ws.numel()]
        variants = {"wgrad alone": lambda: _lib.check(lib.uniir_gemm(C.byref(d), st)),
                    "ln_bwd alone": lambda: _lib.check(lib.uniir_layernorm_bwd_ex(*ln, st)),
                    "two launches": lambda: _lib.check(lib.uniir_gemm_wgrad_ln_bwd(C.byref(d), *ln, 0, st))}
        for c in sides:
            variants[f"fused, {c} side CUs ({lib.uniir_gemm_wgrad_side_plan(rows, tiles, c)} slabs)"] = (
                lambda c=c: _lib.check(lib.uniir_gemm_wgrad_ln_bwd(C.byref(d), *ln, c, st)))
        for fn in variants.values():          # warm-up: code objects, the LDS opt-in
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(REPS):
            for k, fn in variants.items():
                times[k].append(timed(fn))
        print(f"{name}: {rows} rows, dW {M} x {W}, {d.k_splits} splits in the separate launch")
        for k, t in times.items():
            print(f"    {k:36s} median {statistics.median(t):.3f} ms   min {min(t):.3f}   max {max(t):.3f}")
        del A, B


if __name__ == "__main__":
    main()
