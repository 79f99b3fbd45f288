"""The fp32 loss path and the optimizer on every dispatch path against tests/fp32_ref.py.

sgemm (csrc/infonce.hip).  The product is compared bit for bit with the pinned fmaf chain of the CPU oracle on
  S1  sgemm_kernel, 64 x 64 tiles          K % 16 != 0, M or N < 64, M N < 128 * 128 * 8, general strides, a base pointer or a
                                           leading dimension that is no multiple of 4 floats
  S2  sgemm128_kernel<1, 1>                A k-contiguous, B k-contiguous (odd M and N allowed)
  S3  sgemm128_kernel<1, 0>                A k-contiguous, B n-contiguous (N % 4 == 0)
  S4  sgemm128_kernel<0, 1>                A m-contiguous (M % 4 == 0), B k-contiguous
  S5  sgemm128_kernel<0, 0>                both contiguous along the output dimension
  S6  uniir_sgemm_splitk's slab form       per-slice chains added in slice order; `used` < `splits` at K = 1296; its fallbacks
                                           to the plain kernel equal uniir_sgemm bit for bit
each 128-tile instance at ragged M / N edges (261 x 515 where the layout allows odd extents, 260 x 516: three tile rows, the last
with 4 or 5 live rows), one K step and three, scaled (alpha) and accumulating (uniir_sgemm_acc, ldc > N: the padding keeps its NaN
pattern).  alpha_host != 1 is reachable through uniir_sgemm only and a device scale through uniir_infonce_fwd only (which passes
alpha_host = 1), so the two factors are covered apart; fp32_ref.alpha32 restates their product.  An accumulating store with
alpha != 1 may be either of the two forms fp32_ref.sgemm_accepts takes; the OBS line counts them.

InfoNCE: logits bit-exact against the chain; lse, loss and gradients within the bound; hits exact, ties (same thread, neighbouring
lanes, different waves; target first, last, absent) resolved to the first index; dq and d_all_p also bit-exact against the chain of
the kernel's own G.  Hard negatives, softce, select / fuse / pool, AdamW and the EMA: within the bound, += outputs from non-zero
contents, written outputs from a NaN pattern, bf16 shadows bit for bit.  softce sees finite similarities only.
Every test prints its worst |got - ref| / bound as an OBS line."""
import ctypes as C

import numpy as np
import pytest
import torch

import fp32_cases as T
import fp32_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16 = torch.bfloat16
EINVAL, EALIGN = -1, -3
TAIL = 64
Buf = T.Buf


def _lib():
    from uniir_amd import _lib
    return _lib.load()


def _st():
    from uniir_amd import ops
    return ops._stream()


def _p(b, off_bytes=0):
    if b is None:
        return None
    return C.c_void_p((b.view.data_ptr() if isinstance(b, Buf) else b.data_ptr()) + off_bytes)


def _vec(n, fill=None):
    """[n] fp32 with TAIL spare floats behind it; NaN pattern unless filled"""
    b = Buf(1, n, n + TAIL, device=DEV)
    if fill is not None:
        b.set(fill.reshape(1, n) if isinstance(fill, torch.Tensor) else torch.full((1, n), float(fill), device=DEV))
    return b


def _mat(t, dtype=torch.float32):
    return Buf(t.shape[0], t.shape[1], dtype=dtype, device=DEV).set(t)


def _scalar(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def _np(t):
    return t.detach().cpu().contiguous().numpy()


def _check_all(name, got, ref, keys=None):
    ratios = {}
    for k in (keys or got):
        g = got[k].cpu() if isinstance(got[k], torch.Tensor) else torch.as_tensor(got[k])
        r, bnd = ref[k]
        R.check(g.reshape(r.shape), r, bnd, f"{name} {k}")
        ratios[k] = R.worst_ratio(g.reshape(r.shape), r, bnd)
    print(f"\nOBS {name} worst |got - ref| / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


# ======================================================================================================================== sgemm
def _sgemm_call(c, A, B, Cb, entry=None, ws=None, ws_bytes=0):
    (sam, sak, _, _), (sbk, sbn, _, _) = c.strides()
    lib = _lib()
    a = (C.c_void_p(A.flat.data_ptr() + 4 * c.aoff), sam, sak, C.c_void_p(B.flat.data_ptr()), sbk, sbn, _p(Cb), Cb.ld, c.M, c.N, c.K,
         c.alpha)
    entry = entry or c.entry
    if entry == "sgemm":
        return lib.uniir_sgemm(*a, _st())
    if entry == "acc":
        return lib.uniir_sgemm_acc(*a, _st())
    return lib.uniir_sgemm_splitk(*a, int(entry == "splitk_acc"), ws, ws_bytes, _st())


@pytest.mark.parametrize("c", T.SGEMM, ids=[c.name for c in T.SGEMM])
def test_sgemm_path(c):
    A, B, opA, opB = T.sgemm_inputs(c, DEV)
    accumulate = c.entry in ("acc", "splitk_acc")
    Cb = Buf(c.M, c.N, c.N + c.cpad, device=DEV)
    c0 = None
    if accumulate:
        Cb.set(torch.randn(c.M, c.N, device=DEV))
        c0 = _np(Cb.view)
    before = Cb.bits().clone()
    ws = ws_ptr = None
    ws_bytes = 0
    if c.entry.startswith("splitk"):
        need = int(_lib().uniir_sgemm_splitk_workspace_bytes(c.M, c.N, c.K))
        assert need == R.splitk_plan(c.M, c.N, c.K)[0] * c.M * c.N * 4          # sized by splits, not by used
        ws = torch.full((need + 64,), 0x5A, dtype=torch.uint8, device=DEV)
        ws_ptr = C.c_void_p(ws.data_ptr() + (4 if c.ws == "misaligned" else 0))
        ws_bytes = need - 1 if c.ws == "short" else need
    rc = _sgemm_call(c, A, B, Cb, ws=ws_ptr, ws_bytes=ws_bytes)
    torch.cuda.synchronize()
    if c.ws != "ok":
        assert rc == EINVAL, (c.name, rc)
        Cb.assert_all_untouched(before, c.name)
        assert bool((ws == 0x5A).all()), "the refused workspace was written"
        return
    assert rc == 0, (c.name, rc)
    Cb.assert_outside_untouched(before, c.name)
    a, b = _np(opA), _np(opB)
    acc = R.splitk_chain(a, b) if c.path == "S6" else R.chain(a, b)
    got = _np(Cb.view)
    two, fused = R.sgemm_accepts(got, acc, R.alpha32(c.alpha), c0)
    bad = ~(two | fused)
    assert not bad.any(), f"{c.name} ({c.path}): {int(bad.sum())} of {bad.size} elements differ from the chain, first at " \
                          f"{tuple(np.argwhere(bad)[0])}"
    print(f"\nOBS {c.name} {c.path} bitwise against the chain: {bad.size} elements, two-step form {int(two.sum())}, "
          f"fused form {int(fused.sum())}")
    if c.entry.startswith("splitk") and c.path != "S6":          # the fallback is the plain entry point, bit for bit
        C2 = Buf(c.M, c.N, c.N + c.cpad, device=DEV)
        if accumulate:
            C2.set(torch.from_numpy(c0).to(DEV))
        assert _sgemm_call(c, A, B, C2, entry="acc" if accumulate else "sgemm") == 0
        torch.cuda.synchronize()
        assert torch.equal(C2.bits(), Cb.bits())


def test_sgemm_routing_boundary_gives_identical_bits():
    """the same data one column below and at launch_sgemm's M N >= 128 * 128 * 8 threshold: the 64-tile and the 128-tile kernel"""
    above, below = T.BOUNDARY
    A, B, opA, opB = T.sgemm_inputs(above, DEV)
    outs = []
    for c in (above, below):
        Cb = Buf(c.M, c.N, c.N + c.cpad, device=DEV)
        assert _sgemm_call(c, A, B, Cb) == 0          # B's first 511 rows are the smaller problem's operand
        torch.cuda.synchronize()
        outs.append(Cb.view.clone())
    assert torch.equal(outs[0][:, :below.N], outs[1])
    assert np.array_equal(_np(outs[0]), R.chain(_np(opA), _np(opB)))


# ====================================================================================================================== InfoNCE
def _infonce_fwd(q, p, scale, toff):
    b, B, E = q.shape[0], p.shape[0], q.shape[1]
    score, stats, loss, acc = Buf(b, B, device=DEV), _vec(3 * b), _vec(1), _vec(1)
    bufs = (score, stats, loss, acc)
    before = [x.bits().clone() for x in bufs]
    rc = _lib().uniir_infonce_fwd(_p(q), _p(p), _p(scale), b, B, E, toff, _p(score), _p(stats), _p(loss), _p(acc), _st())
    torch.cuda.synchronize()
    assert rc == 0
    for x, was in zip(bufs, before):
        x.assert_outside_untouched(was, "infonce_fwd")
    s = stats.view[0]
    return score.view, {"lse": s[:b], "row_loss": s[b:2 * b], "hit": s[2 * b:], "loss": loss.view[0, 0], "acc": acc.view[0, 0]}


@pytest.mark.parametrize("b,B,E,toff,scale", T.INFONCE)
def test_infonce_path(b, B, E, toff, scale):
    q, p = T.infonce_inputs(b, B, E, DEV)
    sc = _scalar(scale)
    alpha = R.alpha32(1.0, float(sc[0]))
    score, got = _infonce_fwd(q, p, sc, toff)
    want = (R.chain(_np(q), _np(p).T) * alpha).astype(np.float32)
    assert np.array_equal(_np(score), want), "logits differ from the chain"
    ref = R.infonce_fwd(score.cpu(), toff)
    _check_all(f"infonce_fwd {b}x{B}x{E} {T.INFONCE_PATHS[(b, B, E, toff)][0]}", got, ref)
    assert torch.equal(got["hit"].cpu().double(), ref["hit"][0])
    assert round(float(got["acc"]) * b) == int(ref["hit"][0].sum())
    # backward, dloss != 1
    dloss = _scalar(T.DLOSS)
    gbuf, dq, dp, ds = _vec(b * B + b), Buf(b, E, device=DEV), Buf(B, E, device=DEV), _vec(1)
    bufs = (gbuf, dq, dp, ds)
    before = [x.bits().clone() for x in bufs]
    rc = _lib().uniir_infonce_bwd(_p(q), _p(p), _p(sc), _p(score.contiguous()), _p(got["lse"].contiguous()), _p(dloss), b, B, E, toff,
                                  _p(gbuf), _p(dq), _p(dp), _p(ds), _st())
    torch.cuda.synchronize()
    assert rc == 0
    for x, was in zip(bufs, before):
        x.assert_outside_untouched(was, "infonce_bwd")
    G = gbuf.view[0, :b * B].reshape(b, B)
    refb = R.infonce_bwd(q.cpu(), p.cpu(), float(sc[0]), score.cpu(), got["lse"].cpu(), float(dloss[0]), toff)
    paths = T.INFONCE_PATHS[(b, B, E, toff)]
    _check_all(f"infonce_bwd {b}x{B}x{E} dq {paths[1]} d_all_p {paths[2]}",
               {"G": G, "dq": dq.view, "d_all_p": dp.view, "dscale": ds.view[0, 0]}, refb)
    # the two gradient products are the same pinned chains, on the kernel's own G
    assert np.array_equal(_np(dq.view), (R.chain(_np(G), _np(p)) * alpha).astype(np.float32)), "dq differs from the chain"
    assert np.array_equal(_np(dp.view), (R.chain(_np(G).T, _np(q)) * alpha).astype(np.float32)), "d_all_p differs from the chain"


@pytest.mark.parametrize("delta,where", T.TIES)
def test_infonce_argmax_ties_go_to_the_first_index(delta, where):
    q, p, toff, want = T.tie_inputs(delta, where, DEV)
    score, got = _infonce_fwd(q.contiguous(), p.contiguous(), _scalar(1.0), toff)
    assert int((score == score.max()).sum()) == 2, "the two equal maxima"
    assert float(got["hit"][0]) == want and float(got["acc"]) == want
    assert float(R.infonce_fwd(score.cpu(), toff)["hit"][0][0]) == want


# =============================================================================================================== hard negatives
@pytest.mark.parametrize("b,N,I,dim", T.HARDNEG)
def test_hardneg_path(b, N, I, dim):
    q, p, n = T.hardneg_inputs(b, N, I, dim, DEV)
    Cn = 1 + N + I
    sc, dloss = _scalar(14.0), _scalar(T.DLOSS)
    nb = Buf(b * N, dim, device=DEV).set(n.reshape(b * N, dim)) if N else None
    logits, lse, rl, hit = Buf(b, Cn, device=DEV), _vec(b), _vec(b), _vec(b)
    bufs = [logits, lse, rl, hit]
    before = [x.bits().clone() for x in bufs]
    rc = _lib().uniir_hardneg_fwd(_p(q), _p(p), _p(nb), _p(sc), b, N, I, dim, _p(logits), _p(lse), _p(rl), _p(hit), _st())
    torch.cuda.synchronize()
    assert rc == 0
    for x, was in zip(bufs, before):
        x.assert_outside_untouched(was, "hardneg_fwd")
    z = logits.view.cpu()
    ref = R.hardneg_fwd(q.cpu(), p.cpu(), n.cpu(), 14.0, N, I, got_logits=z)
    got = {"logits": z, "lse": lse.view[0], "row_loss": rl.view[0], "hit": hit.view[0]}
    _check_all(f"hardneg_fwd b{b} N{N} I{I} dim{dim}", got, ref)
    assert torch.equal(hit.view[0].cpu().double(), ref["hit"][0])
    if N and b >= 2:
        assert float(hit.view[0, 0]) == 0.0, "row 0: a negative beats the positive"
        assert float(z[1, 0]) == float(z[1, 1]) and float(hit.view[0, 1]) == 1.0, "row 1: a tie goes to index 0"
    # backward: dq / dn written over a NaN pattern, dp / dscale added onto their contents
    dp0 = torch.randn(b, dim, device=DEV)
    dq, dn, dp, ds = Buf(b, dim, device=DEV), (Buf(b * N, dim, device=DEV) if N else None), _mat(dp0), _vec(1, 0.25)
    bufs = [x for x in (dq, dn, dp, ds) if x is not None]
    before = [x.bits().clone() for x in bufs]
    rc = _lib().uniir_hardneg_bwd(_p(q), _p(p), _p(nb), _p(sc), _p(logits), _p(lse), _p(dloss), b, N, I, dim, _p(dq), _p(dp), _p(dn),
                                  _p(ds), _st())
    torch.cuda.synchronize()
    assert rc == 0
    for x, was in zip(bufs, before):
        x.assert_outside_untouched(was, "hardneg_bwd")
    refb = R.hardneg_bwd(q.cpu(), p.cpu(), n.cpu(), 14.0, z, lse.view[0].cpu(), float(dloss[0]), N, I, dp0=dp0.cpu(), dscale0=0.25)
    gotb = {"dq": dq.view, "dp": dp.view, "dscale": ds.view[0, 0]}
    if N:
        gotb["dn"] = dn.view
    assert set(gotb) == set(refb)
    _check_all(f"hardneg_bwd b{b} N{N} I{I} dim{dim}", gotb, refb)


# ======================================================================================================================= softce
@pytest.mark.parametrize("i,n,temp,alpha", [(i,) + c for i, c in enumerate(T.SOFTCE)])
def test_softce_path(i, n, temp, alpha):
    sim, sim_m, ids_row, ids_all, hits = T.softce_inputs(n, DEV)
    b, gscale = T.SOFTCE_B, 0.5
    want_dsim, want_dtemp, dloss = i % 2 == 0, (i // 2) % 2 == 0, (T.DLOSS if i % 3 else None)
    tt = _scalar(temp) if temp is not None else None
    dl = _scalar(dloss) if dloss is not None else None
    rl, hit = _vec(b), _vec(b)
    dsim = Buf(b, n, device=DEV) if want_dsim else None
    dtemp = _vec(b) if want_dtemp else None
    bufs = [x for x in (rl, hit, dsim, dtemp) if x is not None]
    before = [x.bits().clone() for x in bufs]
    rc = _lib().uniir_softce(_p(sim), _p(sim_m), _p(tt), _p(ids_row), _p(ids_all), b, n, alpha, gscale, _p(dl), _p(rl), _p(hit),
                             _p(dsim), _p(dtemp), _st())
    torch.cuda.synchronize()
    assert rc == 0
    for x, was in zip(bufs, before):
        x.assert_outside_untouched(was, "softce")
    ref = R.softce(sim.cpu(), sim_m.cpu(), None if temp is None else float(tt[0]), ids_row.cpu(), ids_all.cpu(), alpha, gscale,
                   None if dloss is None else float(dl[0]))
    got = {"row_loss": rl.view[0], "hit": hit.view[0]}
    if want_dsim:
        got["dsim"] = dsim.view
    if want_dtemp:
        got["row_dtemp"] = dtemp.view[0]
    _check_all(f"softce n{n} temp {temp} alpha {alpha}", got, ref)
    assert torch.equal(hit.view[0].cpu().double(), ref["hit"][0])
    for row, want in hits.items():
        assert float(hit.view[0, row]) == want, f"tie of row {row}"


# ============================================================================================================ select, fuse, pool
@pytest.mark.parametrize("dim", T.SELECT_DIMS)
@pytest.mark.parametrize("with_idx", [True, False])
def test_select_normalize_path(dim, with_idx):
    g = torch.Generator(device=DEV).manual_seed(dim)
    idx = T.select_idx(DEV) if with_idx else None
    nsrc = T.SELECT_SRC if with_idx else T.SELECT_SRC - 1
    rows = T.SELECT_ROWS if with_idx else nsrc
    emb = torch.randn(nsrc, dim, device=DEV, generator=g)
    out, inv = Buf(rows, dim, device=DEV), _vec(rows)
    before = [out.bits().clone(), inv.bits().clone()]
    assert _lib().uniir_select_normalize(_p(emb), _p(idx), _p(out), _p(inv), rows, dim, _st()) == 0
    torch.cuda.synchronize()
    out.assert_outside_untouched(before[0], "out")
    inv.assert_outside_untouched(before[1], "inv_norm")
    ref = R.select_normalize(emb.cpu(), None if idx is None else idx.cpu())
    _check_all(f"select_normalize dim{dim} idx={with_idx}", {"out": out.view, "inv_norm": inv.view[0]}, ref)
    dout = torch.randn(rows, dim, device=DEV, generator=g)
    d0 = torch.randn(nsrc, dim, device=DEV, generator=g)
    demb = _mat(d0)
    was = demb.bits().clone()
    o, iv = out.view.contiguous(), inv.view[0].contiguous()
    assert _lib().uniir_select_normalize_bwd(_p(o), _p(iv), _p(dout), _p(idx), _p(demb), rows, dim, _st()) == 0
    torch.cuda.synchronize()
    demb.assert_outside_untouched(was, "demb")
    refb = R.select_normalize_bwd(o.cpu(), iv.cpu(), dout.cpu(), None if idx is None else idx.cpu(), d0.cpu())
    _check_all(f"select_normalize_bwd dim{dim} idx={with_idx}", {"demb": demb.view}, refb)
    if with_idx:
        assert torch.equal(demb.view[30:], d0[30:]), "an unselected row changed"


@pytest.mark.parametrize("dim", T.FUSE_DIMS)
def test_fuse_embeddings_path(dim):
    txt, img, tm, im, demb = T.fuse_inputs(dim, DEV)
    n = txt.shape[0]
    emb = Buf(n, dim, device=DEV)
    was = emb.bits().clone()
    assert _lib().uniir_fuse_embeddings(_p(txt), _p(img), _p(tm), _p(im), _p(emb), n, dim, _st()) == 0
    torch.cuda.synchronize()
    emb.assert_outside_untouched(was, "emb")
    _check_all(f"fuse_embeddings dim{dim}", {"emb": emb.view}, R.fuse_embeddings(txt.cpu(), img.cpu(), tm.cpu(), im.cpu()))
    dt, di = Buf(n, dim, device=DEV), Buf(n, dim, device=DEV)
    was = [dt.bits().clone(), di.bits().clone()]
    assert _lib().uniir_fuse_embeddings_bwd(_p(demb), _p(tm), _p(im), _p(dt), _p(di), n, dim, _st()) == 0
    torch.cuda.synchronize()
    dt.assert_outside_untouched(was[0], "dtxt")
    di.assert_outside_untouched(was[1], "dimg")
    assert torch.equal(dt.view, demb * tm[:, None].float()) and torch.equal(di.view, demb * im[:, None].float())


@pytest.mark.parametrize("n,Tk,W", T.MEANPOOL)
def test_meanpool_path(n, Tk, W):
    g = torch.Generator(device=DEV).manual_seed(W)
    x = torch.randn(n, Tk, W, device=DEV, generator=g)
    out = Buf(n, W, device=DEV)
    was = out.bits().clone()
    assert _lib().uniir_meanpool_fwd(_p(x), _p(out), n, Tk, W, _st()) == 0
    torch.cuda.synchronize()
    out.assert_outside_untouched(was, "out")
    dout = torch.randn(n, W, device=DEV, generator=g)
    dx = Buf(n * Tk, W, device=DEV)
    was = dx.bits().clone()
    assert _lib().uniir_meanpool_bwd(_p(dout), _p(dx), n, Tk, W, _st()) == 0
    torch.cuda.synchronize()
    dx.assert_outside_untouched(was, "dx")
    _check_all(f"meanpool {n}x{Tk}x{W}", {"out": out.view, "dx": dx.view.reshape(n, Tk, W)},
               {**R.meanpool_fwd(x.cpu()), **R.meanpool_bwd(dout.cpu(), Tk)})


# ==================================================================================================================== optimizer
class _Flat:
    """[count] elements with TAIL spare ones of NaN pattern behind them (Buf's guard rows would double the 16 M case)"""

    def __init__(self, t, dtype=torch.float32):
        self.n = t.numel()
        self.flat = torch.empty(self.n + TAIL, dtype=dtype, device=DEV)
        self.ibits = torch.int32 if dtype == torch.float32 else torch.int16
        self.flat.view(self.ibits).fill_(T.NAN32 if dtype == torch.float32 else T.NAN16)
        self.flat[:self.n].copy_(t)
        self.view = self.flat[:self.n]

    def tail_ok(self):
        return bool((self.flat.view(self.ibits)[self.n:] == (T.NAN32 if self.ibits == torch.int32 else T.NAN16)).all())

    def ptr(self, off=0):
        return C.c_void_p(self.flat.data_ptr() + off)


def _adam_call(P, G, M, V, S, count, wd, step, gs, off=0):
    a = T.ADAM
    return _lib().uniir_adamw_step(P.ptr(off), G.ptr(), M.ptr(), V.ptr(), S.ptr() if S is not None else None, count, a["lr"], a["b1"],
                                   a["b2"], a["eps"], wd, step, gs, _st())


@pytest.mark.parametrize("count", T.ADAMW_COUNTS + (T.ADAMW_BIG,))
def test_adamw_path(count):
    p, g, m, v = T.adamw_inputs(count, DEV)
    P, G, M, V = (_Flat(t) for t in (p, g, m, v))
    S = _Flat(torch.zeros(count, device=DEV), BF16)
    big = count == T.ADAMW_BIG
    plan = T.ADAMW_BIG_PLAN if big else T.ADAMW_PLAN
    worst = {}
    for step, wd, gs, shadow in plan:
        pre = [x.view.clone() for x in (P, M, V)]
        shadow_was = S.view.clone()
        assert _adam_call(P, G, M, V, S if shadow else None, count, wd, step, gs) == 0
        torch.cuda.synchronize()
        # the fp64 step from the state before the call, on the device (the 16 M case in a second)
        ref = R.adamw_step(pre[0], G.view, pre[1], pre[2], wd=wd, step=step, grad_scale=gs, **T.ADAM)
        for k, buf in (("param", P), ("exp_avg", M), ("exp_avg_sq", V)):
            R.check(buf.view, *ref[k], f"adamw count {count} step {step} {k}")
            worst[k] = max(worst.get(k, 0.0), R.worst_ratio(buf.view, *ref[k]))
        if shadow:
            assert torch.equal(S.view.view(torch.int16), P.view.to(BF16).view(torch.int16)), "the bf16 shadow is not bf16(param)"
        else:
            assert torch.equal(S.view.view(torch.int16), shadow_was.view(torch.int16)), "a shadow that was not passed changed"
        del ref, pre
    assert all(x.tail_ok() for x in (P, G, M, V, S)), "written behind count"
    print(f"\nOBS adamw count {count} worst |got - ref| / bound: " + ", ".join(f"{k} {r:.3f}" for k, r in worst.items()))


def test_adamw_and_ema_alignment_errors():
    p, g, m, v = T.adamw_inputs(1006, DEV)
    P, G, M, V = (_Flat(t) for t in (p, g, m, v))
    was = P.flat.clone()
    assert _adam_call(P, G, M, V, None, 1000, 0.2, 1, 1.0, off=4) == EALIGN
    S = _Flat(torch.zeros(1006, device=DEV), BF16)
    a = T.ADAM
    rc = _lib().uniir_adamw_step(P.ptr(), G.ptr(), M.ptr(), V.ptr(), S.ptr(2), 1000, a["lr"], a["b1"], a["b2"], a["eps"], 0.2, 1, 1.0,
                                 _st())
    assert rc == EALIGN
    assert _lib().uniir_ema_update(P.ptr(), G.ptr(), None, 1006, 0.995, _st()) == EALIGN          # count % 4
    assert _lib().uniir_ema_update(P.ptr(4), G.ptr(), None, 1000, 0.995, _st()) == EALIGN
    torch.cuda.synchronize()
    assert torch.equal(P.flat.view(torch.int32), was.view(torch.int32))


@pytest.mark.parametrize("shadow", [False, True])
def test_ema_update_path(shadow):
    count = T.EMA_COUNT
    pm, p, _, _ = T.adamw_inputs(count, DEV, seed=3)
    PM, P = _Flat(pm), _Flat(p)
    S = _Flat(torch.zeros(count, device=DEV), BF16)
    assert _lib().uniir_ema_update(PM.ptr(), P.ptr(), S.ptr() if shadow else None, count, T.EMA_MOMENTUM, _st()) == 0
    torch.cuda.synchronize()
    ref = R.ema_update(pm, p, T.EMA_MOMENTUM)
    R.check(PM.view, *ref["param_m"], "ema")
    assert torch.equal(P.view, p) and PM.tail_ok() and S.tail_ok()
    if shadow:
        assert torch.equal(S.view.view(torch.int16), PM.view.to(BF16).view(torch.int16))
    else:
        assert not bool(S.view.any())
    print(f"\nOBS ema shadow={shadow} worst |got - ref| / bound: param_m {R.worst_ratio(PM.view, *ref['param_m']):.3f}")
