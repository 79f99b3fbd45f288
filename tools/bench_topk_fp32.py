"""The fp32 candidate-pool search (uniir_topk_ip_f32) beside the fp16 search (uniir_topk_ip) of the SAME rows -- x.half() and x -- in one
process, alternating (dev tool; no number is a target, the output is the record the documents quote).  The parent has no fp32 search:
the fp16 search of the same rows is the yardstick.
Per shape (rows x 768, nq queries, k = 10): one warm-up of each dtype, then RUNS runs of ITERS searches each, dtypes alternating,
device events around every search, the median of a run; both runs are printed (their spread is the error bar).  Bytes and FLOPs
come from the shapes: one sweep of <= 256 (fp16) / <= 1024 (fp32) queries reads every row once; the scan does 2 * nq * rows * dim
FLOP.  Roofs used to name the binding one: 6.29 TB/s of HBM as measured by the scans here, 155 TFLOP/s of v_mfma_f32_16x16x4_f32
and 2.5 PFLOP/s of the fp16 MFMA (the microarchitecture notes DESIGN.md quotes).
    python tools/bench_topk_fp32.py [--rows 262144,699040] [--queries 1,64,256,1024] [--iters 5] [--runs 2] [--out profiles/topk_fp32.txt]"""
import argparse
import os
import socket
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

HBM_TBS, F32_TF, F16_TF = 6.29, 155.0, 2500.0


def _run(search, iters):
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        search()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="262144,699040")
    ap.add_argument("--queries", default="1,64,256,1024")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_topk_fp32.py measures on the GPU; there is none here")
    from uniir_amd import retrieval
    out = open(a.out, "a") if a.out else None

    def say(line):
        print(line, flush=True)
        if out is not None:
            out.write(line + "\n")
            out.flush()

    say(f"device: {torch.cuda.get_device_name(0)}  box: {socket.gethostname()}  clock: {time.strftime('%Y-%m-%d %H:%M:%S %Z')}")
    say(f"dim {a.dim}, k {a.k}, {a.iters} searches per run (median), {a.runs} runs, fp16 and fp32 alternating; ms per search")
    dim = a.dim
    for rows in [int(r) for r in a.rows.split(",") if r]:
        g = torch.Generator(device="cuda").manual_seed(rows)
        x = torch.randn(rows, dim, device="cuda", generator=g) * 0.3
        ids = torch.arange(rows, device="cuda", dtype=torch.int64)
        shards = {"fp16": retrieval.PoolShard(x.half(), ids), "fp32": retrieval.PoolShard(x, ids)}
        del x
        for nq in [int(q) for q in a.queries.split(",") if q]:
            q = torch.randn(nq, dim, device="cuda", generator=g)
            qs = {"fp16": q.half(), "fp32": q}
            fn = {p: (lambda p=p: retrieval.search_shard(shards[p], qs[p], a.k)) for p in ("fp16", "fp32")}
            i16, i32 = fn["fp16"]()[1], fn["fp32"]()[1]          # warm-up of both shapes
            torch.cuda.synchronize()
            same = float((i16 == i32).all(dim=1).float().mean())
            ms = {"fp16": [], "fp32": []}
            for _ in range(a.runs):
                for p in ("fp16", "fp32"):
                    ms[p].append(_run(fn[p], a.iters))
            line = f"  rows {rows:7d} nq {nq:5d}:"
            best = {}
            for p, item, sweep, peak in (("fp16", 2, retrieval.sweep_queries(dim, rows), F16_TF), ("fp32", 4, 1024, F32_TF)):
                sweeps = -(-nq // sweep)
                gb = sweeps * rows * dim * item / 1e9
                gf = 2.0 * nq * rows * dim / 1e9
                t_hbm, t_mfma = gb / HBM_TBS, gf / peak                  # ms (GB / (TB/s) = ms; GFLOP / (TFLOP/s) = ms)
                best[p] = min(ms[p])
                roof = "HBM" if t_hbm >= t_mfma else "MFMA"
                line += (f"  {p} " + " / ".join(f"{t:.3f}" for t in ms[p]) + f" ms ({gb:.2f} GB, {gf:.1f} GFLOP; roof {roof} "
                         f"{max(t_hbm, t_mfma):.3f} ms = {100 * max(t_hbm, t_mfma) / best[p]:.0f} % of it)")
            say(line + f"  fp32 / fp16 {best['fp32'] / best['fp16']:.2f}; queries whose top-{a.k} ids agree {100 * same:.0f} %")
        del shards
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
