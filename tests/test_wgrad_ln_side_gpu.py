"""uniir_gemm_wgrad_ln_bwd (include/uniir_hip.h; csrc/gemm.hip gemm_wgrad_side_kernel, csrc/ln_row.h): a weight gradient and an
independent LayerNorm backward in one launch, against the two entry points it replaces and against the fp64 references.

Kernel level.  The grid: LayerNorm width 512 / 768 / 1024 x rows 3 / 4096 / 4100 / 8231 (fewer rows than side waves, an exact count,
a K tail of the product, a strided row loop) x dW 256 x 256 / 512 x 768 / 1024 x 3072 x side units 0 / 32 / 48 x every option on
(dres, branch_scale, dx_colsum, a_rowsum) and off.  No product of that grid has a chunk plan (224 and 208 workgroups need 7 or 13 to
divide tiles x splits: uniir_gemm_wgrad_side_plan), so the grid pins the contract "the call IS the two launches"; FUSED adds the
smallest shapes that do have a plan, one per chunk count: 3, 4, 7 (two chunks per workgroup) and 13 slabs (three chunks per
workgroup, with the row sums), with and without a K tail, at each width.  test_fused_cases_run_the_side_kernel asserts from the
profiler that these launch gemm_wgrad_side_kernel and the grid does not.
Expected: dx_f32 / dx_bf16 bitwise uniir_layernorm_bwd_ex's; dgamma / dbeta / dx_colsum within tests/fp32_ref.py's bound and bitwise
equal between two runs; dW (and the row sums) bitwise uniir_gemm's at the same split count with the same slab workspace, within
tests/gemm_ref.py's bound, and bitwise equal between two runs.

Tower level.  The 3 + 3-layer CLIP of tests/test_recompute_gpu.py, clip_model.ln_bwd_side on against off: loss and embeddings equal,
every parameter gradient within 1e-4 relative norm (two valid orders of the same fp32 sums), two runs with the flag on bitwise equal.
At that size no pair has a plan either, so the flag's two launch orders are compared; test_tower_with_a_fused_pair makes the same
comparison on a vision tower whose c_fc pair does fuse (width 512, 13 320 rows)."""
import ctypes as C
import functools
import itertools
import os
import sys

import pytest
import torch

import fp32_ref as LR
import gemm_ref as GR

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
EPS = 1e-5
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uniir_amd", "src"))


def _lib():
    from uniir_amd import _lib
    return _lib


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@functools.lru_cache(maxsize=None)
def _workspace():
    return torch.empty(13 * 3072 * 1024 * 4 + 4096, dtype=torch.uint8, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- shared inputs
@functools.lru_cache(maxsize=None)
def _ln_inputs(rows, width):
    g = torch.Generator(device=DEV).manual_seed(1000 * width + rows)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)          # noqa: E731
    x = r(rows, width) * 1.5 + 0.25
    return dict(x=x, gamma=1.0 + 0.1 * r(width), dy=r(rows, width).to(BF16), dres=r(rows, width),
                bscale=(torch.rand(rows, device=DEV, generator=g) < 0.7).float() / 0.7,
                dgamma0=r(width), dbeta0=r(width), colsum0=r(width))


@functools.lru_cache(maxsize=None)
def _gemm_inputs(rows, M, N):
    g = torch.Generator(device=DEV).manual_seed(7 * rows + M + N)
    A = torch.randn(rows, M, device=DEV, generator=g).to(BF16)                              # dy of the layer, K-major
    B = (torch.randn(rows, N, device=DEV, generator=g) / max(1.0, rows ** 0.5)).to(BF16)      # its input
    return dict(A=A, B=B, c0=torch.randn(M, N, device=DEV, generator=g), rowsum0=torch.randn(M, device=DEV, generator=g))


@functools.lru_cache(maxsize=None)
def _ln_reference(rows, width, opts):
    d = _ln_inputs(rows, width)
    ref = LR.norm_bwd(d["x"], d["gamma"], d["dy"], EPS, False, dres=d["dres"] if opts else None,
                      branch_scale=d["bscale"] if opts else None, dgamma0=d["dgamma0"], dbeta0=d["dbeta0"],
                      colsum0=d["colsum0"] if opts else None)
    return {k: ref[k] for k in ("dgamma", "dbeta", "dx_colsum") if k in ref}


@functools.lru_cache(maxsize=None)
def _gemm_reference(rows, M, N, opts):
    d = _gemm_inputs(rows, M, N)
    return GR.gemm_reference(d["A"].t(), d["B"], epilogue=GR.EPI_ATOMIC_F32, c0=d["c0"], rowsum0=d["rowsum0"] if opts else None)


# ---------------------------------------------------------------------------------------------------------------------- one call
class _Call:
    def __init__(self, rows, width, M, N, opts):
        self.rows, self.width, self.M, self.N, self.opts = rows, width, M, N, opts
        ln, gm = _ln_inputs(rows, width), _gemm_inputs(rows, M, N)
        self.ln, self.gm = ln, gm
        self.dx = torch.full((rows, width), float("nan"), device=DEV)
        self.dxb = torch.full((rows, width), float("nan"), device=DEV, dtype=BF16)
        self.dgamma, self.dbeta = ln["dgamma0"].clone(), ln["dbeta0"].clone()
        self.colsum = ln["colsum0"].clone() if opts else None
        self.dW = gm["c0"].clone()
        self.rowsum = gm["rowsum0"].clone() if opts else None

    def desc(self, splits):
        from uniir_amd import ops
        d = _lib().GemmDesc()
        d.A, d.B, d.C = self.gm["A"].data_ptr(), self.gm["B"].data_ptr(), self.dW.data_ptr()
        d.M, d.N, d.K = self.M, self.N, self.rows
        d.lda, d.ldb, d.ldc = self.M, self.N, self.N
        d.a_tmaj = d.b_tmaj = 1
        d.epilogue, d.act, d.dtype, d.alpha = GR.EPI_ATOMIC_F32, 0, 0, 1.0
        d.k_splits = splits
        d.splitk_ws, d.splitk_ws_bytes = _workspace().data_ptr(), _workspace().numel()
        d.a_rowsum = self.rowsum.data_ptr() if self.rowsum is not None else None
        return d

    def ln_args(self):
        ln, o = self.ln, self.opts
        return (_p(ln["x"]), self.width, _p(ln["gamma"]), _p(ln["dy"]), 0, _p(ln["dres"]) if o else None, _p(self.dx), self.width,
                _p(self.dxb), _p(self.dgamma), _p(self.dbeta), _p(self.colsum), _p(ln["bscale"]) if o else None, self.rows, self.width,
                EPS)

    def outputs(self):
        out = dict(dx_f32=self.dx, dx_bf16=self.dxb, dgamma=self.dgamma, dbeta=self.dbeta, dW=self.dW)
        if self.opts:
            out.update(dx_colsum=self.colsum, rowsum=self.rowsum)
        return out


def _tiles(M, N):
    return -(-M // 256) * -(-N // 256)


def _run_fused(rows, width, M, N, side, opts):
    from uniir_amd import ops
    lib, st = _lib().load(), ops._stream()
    c = _Call(rows, width, M, N, opts)
    d = c.desc(lib.uniir_gemm_wgrad_splits(rows, _tiles(M, N)))
    rc = lib.uniir_gemm_wgrad_ln_bwd(C.byref(d), *c.ln_args(), side, st)
    torch.cuda.synchronize()
    assert rc == 0, lib.uniir_strerror(rc)
    return c


def _run_separate(rows, width, M, N, splits, opts):
    from uniir_amd import ops
    lib, st = _lib().load(), ops._stream()
    c = _Call(rows, width, M, N, opts)
    d = c.desc(splits)
    assert lib.uniir_gemm(C.byref(d), st) == 0
    assert lib.uniir_layernorm_bwd_ex(*c.ln_args(), st) == 0
    torch.cuda.synchronize()
    return c


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF16 else torch.int32)


def _check(rows, width, M, N, side, opts):
    lib = _lib().load()
    plan = lib.uniir_gemm_wgrad_side_plan(rows, _tiles(M, N), side)
    got = _run_fused(rows, width, M, N, side, opts)
    # the split count the product ran with: the plan's, or -- the two launches -- the descriptor's
    want = _run_separate(rows, width, M, N, plan if plan else lib.uniir_gemm_wgrad_splits(rows, _tiles(M, N)), opts)
    g, w = got.outputs(), want.outputs()
    lnref, gref = _ln_reference(rows, width, opts), _gemm_reference(rows, M, N, opts)
    ratios = {k: LR.worst_ratio(g[k], *lnref[k]) for k in lnref}
    ratios["dW"] = LR.worst_ratio(g["dW"], *gref["C"])
    if opts:
        ratios["rowsum"] = LR.worst_ratio(g["rowsum"], *gref["rowsum"])
    same = {k: bool(torch.equal(_bits(g[k]), _bits(w[k]))) for k in g}
    print(f"\nOBS rows {rows} width {width} dW {M}x{N} side {side} opts {int(opts)} plan {plan}: worst |got - ref| / bound "
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + "; bitwise equal to the two launches: "
          + ", ".join(k for k, v in same.items() if v))
    for k in ("dx_f32", "dx_bf16"):
        assert same[k], f"{k} differs from uniir_layernorm_bwd_ex"
    assert bool(torch.isfinite(g["dx_f32"]).all())
    for k in lnref:
        LR.check(g[k], *lnref[k], k)
    assert same["dW"], "dW differs from uniir_gemm at the same split count"
    GR.check(g["dW"], *gref["C"], "dW")
    if opts:
        assert same["rowsum"], "the row sums differ from uniir_gemm's at the same split count"
        GR.check(g["rowsum"], *gref["rowsum"], "rowsum")
    again = _run_fused(rows, width, M, N, side, opts).outputs()
    for k in g:
        assert torch.equal(_bits(again[k]), _bits(g[k])), f"{k} differs between two runs"
    return plan


GRID = list(itertools.product((512, 768, 1024), (3, 4096, 4100, 8231), ((256, 256), (512, 768), (1024, 3072)), (0, 32, 48), (False, True)))
# (rows, width, M, N, side units, options, plan): the smallest products with a chunk plan
FUSED = [(4100, 512, 4096, 1024, 64, True, 3),        # 64 tiles x 3 = 192 x 1, K tail of 4 rows
         (4096, 768, 3072, 1024, 64, False, 4),       # 48 tiles x 4 = 192 x 1
         (4100, 1024, 1024, 3072, 64, True, 4),
         (8100, 1024, 4096, 1024, 32, True, 7),       # 64 tiles x 7 = 224 x 2, K tail of 36 rows
         (8064, 512, 1024, 4096, 32, False, 7),
         (13350, 1024, 3072, 1024, 48, True, 13),     # 48 tiles x 13 = 208 x 3, K tail of 38 rows
         (13312, 768, 3072, 1024, 48, False, 13)]


@pytest.mark.parametrize("width,rows,shape,side,opts", GRID,
                         ids=[f"w{w}-r{r}-{s[0]}x{s[1]}-c{c}-{'opts' if o else 'plain'}" for w, r, s, c, o in GRID])
def test_grid_is_the_two_launches(width, rows, shape, side, opts):
    assert _check(rows, width, shape[0], shape[1], side, opts) == 0


@pytest.mark.parametrize("rows,width,M,N,side,opts,plan", FUSED, ids=[f"r{c[0]}-w{c[1]}-{c[2]}x{c[3]}-c{c[4]}-s{c[6]}" for c in FUSED])
def test_fused_launch(rows, width, M, N, side, opts, plan):
    assert _check(rows, width, M, N, side, opts) == plan


def _kernel_names(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sorted({e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA})


def test_fused_cases_run_the_side_kernel():
    rows, width, M, N, side, opts, _ = FUSED[3]
    fused = _kernel_names(lambda: _run_fused(rows, width, M, N, side, opts))
    print("\n".join(fused))
    assert any("gemm_wgrad_side_kernel" in n for n in fused), fused
    assert not any("ln_bwd_kernel" in n or "gemm_glds_kernel" in n for n in fused), fused
    two = _kernel_names(lambda: _run_fused(8231, 1024, 1024, 3072, 48, True))
    assert not any("gemm_wgrad_side_kernel" in n for n in two), two
    assert any("ln_bwd_kernel" in n for n in two) and any("gemm_glds_kernel" in n for n in two), two


def test_without_slab_room_the_call_is_the_two_launches():
    """a workspace one byte short of the plan's slabs: same results as uniir_gemm with that descriptor + uniir_layernorm_bwd_ex"""
    from uniir_amd import ops
    lib, st = _lib().load(), ops._stream()
    rows, width, M, N, side, opts, plan = FUSED[3]
    outs = []
    for fused in (True, False):
        c = _Call(rows, width, M, N, opts)
        d = c.desc(lib.uniir_gemm_wgrad_splits(rows, _tiles(M, N)))
        d.splitk_ws_bytes = plan * M * N * 4 - 1
        if fused:
            assert lib.uniir_gemm_wgrad_ln_bwd(C.byref(d), *c.ln_args(), side, st) == 0
        else:
            assert lib.uniir_gemm(C.byref(d), st) == 0 and lib.uniir_layernorm_bwd_ex(*c.ln_args(), st) == 0
        torch.cuda.synchronize()
        outs.append(c.outputs())
    for k in outs[0]:
        assert torch.equal(_bits(outs[0][k]), _bits(outs[1][k])), k


# ------------------------------------------------------------------------------------------------------------------------- tower
def _tower_step(cfg, pairs, side, seed=5):
    """loss, embeddings and every parameter gradient of one train-mode forward + backward of a small CLIP_SF"""
    from types import SimpleNamespace
    from oracle import clip_oracle as O
    from uniir_amd import clip_model
    from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
    clip_model.CLIP_CONFIGS["tiny-side"] = cfg
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    model = CLIPScoreFusion("tiny-side", device=DEV, config=config)
    clip = model.clip_model
    clip.load_state_dict(O.init_state_dict(cfg, seed=seed), strict=True)
    clip.ln_bwd_side = side
    model.train()
    batch = O.synthetic_batch(cfg, pairs, seed=33)
    dbatch = {k: (v.to(DEV) if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    clip._ensure_flat()
    clip.zero_grad()
    temb, iemb = clip.encode_text(dbatch["txt_batched"]), clip.encode_image(dbatch["image_batched"])
    out = model(dbatch)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in clip.named_parameters() if p.grad is not None}
    return dict(loss=float(out["loss"].detach()), temb=temb.detach().clone(), iemb=iemb.detach().clone(), grads=grads)


def _compare_flag(cfg, pairs):
    off, on, on2 = _tower_step(cfg, pairs, False), _tower_step(cfg, pairs, True), _tower_step(cfg, pairs, True)
    assert on["loss"] == off["loss"] == on2["loss"]
    for k in ("temb", "iemb"):
        assert torch.equal(on[k], off[k]), k
    assert set(on["grads"]) == set(off["grads"]) and len(off["grads"]) > 20
    worst = ("", 0.0)
    for n, g in off["grads"].items():
        rel = float((on["grads"][n].double() - g.double()).norm() / g.double().norm().clamp_min(1e-30))
        worst = max(worst, (n, rel), key=lambda t: t[1])
        assert rel <= 1e-4, (n, rel)
        assert torch.equal(on["grads"][n], on2["grads"][n]), f"{n} differs between two runs with the flag on"
    print(f"\nOBS worst relative gradient difference, flag on vs off: {worst[1]:.3e} ({worst[0]})")


def test_tower_flag_on_equals_flag_off():
    """the 3 + 3-layer configuration of tests/test_recompute_gpu.py (width 128: no pair has a plan, the flag moves the two
    activation-gradient GEMMs in front of their layers' weight gradients)"""
    from oracle import clip_oracle as O
    _compare_flag(O.tiny_config(vision_width=128, vision_layers=3, transformer_width=128, transformer_heads=2, transformer_layers=3), 24)


def test_tower_with_a_fused_pair():
    """a vision tower in which the c_fc pair does fuse: width 512, 37 tokens, 360 images = 13 320 rows (208 K steps: 13 slabs of 16 on
    208 workgroups, one chunk each, beside 48 side workgroups); the first of its two blocks is a full block (the last runs pooled).
    Same comparison, and the profiler sees the side kernel with the flag on only."""
    from oracle import clip_oracle as O
    cfg = O.tiny_config(vision_width=512, vision_layers=2, image_resolution=96, vision_patch_size=16, transformer_width=128,
                        transformer_heads=2, transformer_layers=2)
    assert _lib().load().uniir_gemm_wgrad_side_plan(360 * 37, 16, 48) == 13
    _compare_flag(cfg, 180)
    for side in (True, False):
        names = _kernel_names(lambda: _tower_step(cfg, 180, side))
        assert any("gemm_wgrad_side_kernel" in n for n in names) == side, (side, names)
