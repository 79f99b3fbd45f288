"""tests/fp32_ref.py tested on the CPU: a bound that cannot fail is worthless.

  * every fp64 reference agrees with torch.autograd in float64 on the same formula (1e-12 relative) and with the committed goldens
    G1 / G3 at the tolerances tests/test_parity_exact_gpu.py uses for them;
  * a plain torch float32 restatement of every operation, summed in another order than the kernel's, stays inside every bound with
    zero violations for every case of the GPU tables (tests/fp32_cases.py) at its real shape, and no closer to it than half: a ratio
    above 0.5 would mean a bound that is too tight or a wrong derivation;
  * eleven planted defects of the restatements each violate a bound, and so does one row lost from the 8231-row column sums;
  * the restated host arithmetic (ln_nc / EXACT, launch_sgemm's `big`, the split-K plan) sends every GPU case to the path it names.
"""
import os
from collections import defaultdict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_cases as T
import fp32_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RATIOS = defaultdict(float)
BF16 = torch.bfloat16


def _check(op, got, ref_bound, what):
    ref, bound = ref_bound
    R.check(got, ref, bound, what)
    r = R.worst_ratio(got, ref, bound)
    assert r <= 0.5, f"{what}: a correct fp32 restatement at {r:.3f} of its bound -- the bound is too tight or its derivation wrong"
    RATIOS[op] = max(RATIOS[op], r)


def _close(a, b, what, rel=1e-12):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    err = float((a - b).abs().max())
    assert err <= rel * max(1.0, float(b.abs().max())), (what, err)


def s32(t, dim=-1):
    """fp32 sum in another order than the kernels': the two halves of the extent, each by torch's own blocked sum"""
    n = t.shape[dim]
    h = n // 2
    return t.narrow(dim, 0, h).sum(dim) + t.narrow(dim, h, n - h).sum(dim)


# ======================================================================================================== fp32 restatements
def norm_fwd32(x, g, b, eps, rms, defect=None):
    W = x.shape[1]
    if rms:
        mean = 0.0
    else:
        xs = x[:, :-1] if defect == "drop_column" else x
        div = 256 * R.ln_path(W)[0] if defect == "padded_mean" else W
        mean = s32(xs)[:, None] / div
    xc = x - mean
    rstd = 1.0 / torch.sqrt(s32(xc * xc)[:, None] / W + eps)
    y = xc * rstd * g
    if not rms or defect == "rms_beta":
        y = y + b
    return {"y_f32": y, "y_bf16": y.to(BF16)}


def norm_bwd32(c, d, defect=None):
    x, g, W = d["x"], d["gamma"], c.width
    dy = d["dy"].float()
    mean = 0.0 if c.rms else s32(x)[:, None] / W
    xc = x - mean
    rstd = 1.0 / torch.sqrt(s32(xc * xc)[:, None] / W + c.eps)
    xhat = xc * rstd
    gg = dy * g
    c1 = 0.0 if c.rms else s32(gg)[:, None] / W
    c2 = s32(gg * xhat)[:, None] / W
    dx = (gg - c1 - xhat * c2) * rstd
    if "dres" in d:
        dres = d["dres"]
        if defect == "dres_stride":          # stored with dx_stride, read with width
            buf = T.Buf(c.rows, W, c.dx_stride).set(dres)
            dres = buf.flat.as_strided((c.rows, W), (W, 1))
        dx = dx + dres
    bs = d.get("branch_scale")
    sdx = dx if bs is None else dx * bs[:, None]
    out = {"dx_f32": sdx if defect == "scale_dx_f32" else dx, "dx_bf16": sdx.to(BF16)}
    rs = lambda t: s32(t, 0)          # noqa: E731
    out["dgamma"] = rs(dy * xhat) if defect == "dgamma_overwrite" else d["dgamma0"] + rs(dy * xhat)
    if not c.rms:
        out["dbeta"] = d["dbeta0"] + rs(dy)
    if "colsum0" in d:
        out["dx_colsum"] = d["colsum0"] + rs(sdx)
    return out


def _argmax32(z, last=False):
    if last:
        return z.shape[1] - 1 - R._first_argmax(z.flip(1))
    return R._first_argmax(z)


def infonce_fwd32(z, toff, defect=None):
    b = z.shape[0]
    t = toff + torch.arange(b) + (1 if defect == "target_off" else 0)
    lse = torch.logsumexp(z, 1)
    rl = lse - z[torch.arange(b), t]
    hit = (_argmax32(z, defect == "argmax_last") == t).float()
    return {"lse": lse, "row_loss": rl, "hit": hit, "loss": s32(rl, 0) / b, "acc": s32(hit, 0) / b}


def infonce_bwd32(q, p, scale, z, lse, dloss, toff):
    b, B = z.shape
    G = torch.exp(z - lse[:, None])
    G[torch.arange(b), toff + torch.arange(b)] -= 1.0
    G = G * np.float32(dloss / b)
    s = np.float32(scale)
    return {"G": G, "dq": (G @ p) * s, "d_all_p": (G.t() @ q) * s, "dscale": s32(s32(G * z), 0) / s}


def hardneg32(q, p, n, scale, N, I, dloss, dp0, ds0):
    b, dim = q.shape
    V = R._hn_vectors(p, n if N else None, N, I)
    s = np.float32(scale)
    z = s32(q[:, None, :] * V) * s
    lse = torch.logsumexp(z, 1)
    fwd = {"logits": z, "lse": lse, "row_loss": lse - z[:, 0], "hit": (R._first_argmax(z) == 0).float()}
    D = torch.exp(z - lse[:, None])
    D[:, 0] -= 1.0
    D = D * np.float32(dloss / b)
    dl = D * s
    own = torch.ones(1 + N + I, dtype=torch.bool)
    own[1:1 + N] = False
    bwd = {"dq": (dl[:, :, None] * V).sum(1), "dp": dp0 + dl[:, own].sum(1, keepdim=True) * q,
           "dscale": torch.tensor(ds0) + s32(s32(D * z), 0) / s}
    if N:
        bwd["dn"] = dl[:, 1:1 + N, None] * q[:, None, :]
    return fwd, bwd


def softce32(sim, sim_m, temp, ids_row, ids_all, alpha, gscale, dloss, defect=None):
    Tt = np.float32(1.0 if temp is None else temp)
    z, zm = sim / Tt, sim_m / Tt
    pos = (ids_all[None, :] == ids_row[:, None]).float()
    npos = torch.full_like(pos[:, :1], pos.shape[1]) if defect == "inv_pos_n" else pos.sum(1, keepdim=True)
    inv_pos = torch.where(pos.sum(1, keepdim=True) > 0, 1.0 / npos, torch.zeros_like(npos))
    tgt = np.float32(alpha) * torch.softmax(zm, 1) + (1 - np.float32(alpha)) * pos * inv_pos
    lsm = torch.log_softmax(z, 1)
    gs = np.float32(gscale) * np.float32(1.0 if dloss is None else dloss)
    g = (torch.exp(lsm) - tgt) * gs
    hit = pos[torch.arange(z.shape[0]), R._first_argmax(z)]
    return {"row_loss": -s32(lsm * tgt), "hit": hit, "dsim": g / Tt, "row_dtemp": -s32(g * z) / Tt}


def select_bwd32(out, inv, dout, idx, demb0, defect=None):
    t = (dout - out * s32(out * dout)[:, None]) * inv[:, None]
    demb = demb0.clone()
    idx = torch.arange(out.shape[0]) if idx is None else idx.long()
    if defect == "dup_once":
        demb[idx] += t              # advanced-index +=: a repeated destination is written once
    else:
        demb.index_add_(0, idx, t)
    return {"demb": demb}


def adamw32(p, g, m, v, lr, b1, b2, eps, wd, step, gs, defect=None):
    f = np.float32
    st = step - 1 if defect == "bias_step" else step
    bc1 = f(1) - f(b1) ** f(st)
    bc2s = np.sqrt(f(1) - f(b2) ** f(st))
    g1 = g * f(gs)
    m1 = m * f(b1) + g1 * (f(1) - f(b1))
    v1 = v * f(b2) + g1 * g1 * (f(1) - f(b2))
    p1 = p * (f(1) - f(lr) * f(wd))
    p1 = p1 - (f(lr) / bc1) * (m1 / (torch.sqrt(v1) / bc2s + f(eps)))
    return {"param": p1, "exp_avg": m1, "exp_avg_sq": v1}


# ============================================================================================== fp64 references against autograd
@pytest.mark.parametrize("rms", [False, True])
def test_norm_reference_against_autograd(rms):
    torch.manual_seed(1)
    R_, W, eps = 7, 260, 1e-5
    x = torch.randn(R_, W, dtype=torch.float64, requires_grad=True)
    g = torch.randn(W, dtype=torch.float64, requires_grad=True)
    b = torch.randn(W, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(R_, W, dtype=torch.float64)
    if rms:
        y = g * x * torch.rsqrt((x * x).mean(1, keepdim=True) + eps)
    else:
        y = F.layer_norm(x, (W,), g, b, eps)
    (y * dy).sum().backward()
    _close(R.norm_fwd(x.detach(), g.detach(), b.detach(), eps, rms)["y_f32"][0], y.detach(), "y")
    o = R.norm_bwd(x.detach(), g.detach(), dy, eps, rms)
    _close(o["dx_f32"][0], x.grad, "dx")
    _close(o["dgamma"][0], g.grad, "dgamma")
    if not rms:
        _close(o["dbeta"][0], b.grad, "dbeta")
    # the options: dres is added, branch_scale scales dx_bf16 and dx_colsum only, the sums start from their prior contents
    dres, bs, p0 = torch.randn(R_, W, dtype=torch.float64), torch.rand(R_, dtype=torch.float64), torch.randn(W, dtype=torch.float64)
    o2 = R.norm_bwd(x.detach(), g.detach(), dy, eps, rms, dres=dres, branch_scale=bs, dgamma0=p0, dbeta0=p0, colsum0=p0)
    _close(o2["dx_f32"][0], x.grad + dres, "dx + dres")
    _close(o2["dx_bf16"][0], (x.grad + dres) * bs[:, None], "scaled dx")
    _close(o2["dx_colsum"][0], p0 + ((x.grad + dres) * bs[:, None]).sum(0), "colsum")
    _close(o2["dgamma"][0], p0 + g.grad, "dgamma +=")


def test_infonce_reference_against_autograd():
    torch.manual_seed(2)
    b, B, E, toff, s0, dloss = 5, 9, 8, 3, 14.0, 0.37
    q = torch.randn(b, E, dtype=torch.float64, requires_grad=True)
    p = torch.randn(B, E, dtype=torch.float64, requires_grad=True)
    s = torch.tensor(s0, dtype=torch.float64, requires_grad=True)
    z = q @ p.t() * s
    z.retain_grad()
    t = toff + torch.arange(b)
    loss = F.cross_entropy(z, t)
    (dloss * loss).backward()
    f = R.infonce_fwd(z.detach(), toff)
    _close(f["loss"][0], loss.detach(), "loss")
    _close(f["lse"][0], torch.logsumexp(z.detach(), 1), "lse")
    _close(f["acc"][0], (z.detach().argmax(1) == t).double().mean(), "acc")
    o = R.infonce_bwd(q.detach(), p.detach(), s0, z.detach(), f["lse"][0], dloss, toff)
    for k, want in (("G", z.grad), ("dq", q.grad), ("d_all_p", p.grad), ("dscale", s.grad)):
        _close(o[k][0], want, k)


def test_hardneg_reference_against_autograd():
    torch.manual_seed(3)
    b, N, I, dim, s0, dloss = 5, 3, 2, 8, 7.0, 0.37
    q, p = (torch.randn(b, dim, dtype=torch.float64, requires_grad=True) for _ in range(2))
    n = torch.randn(b, N, dim, dtype=torch.float64, requires_grad=True)
    s = torch.tensor(s0, dtype=torch.float64, requires_grad=True)
    V = torch.cat([p[:, None], n, p[:, None].expand(b, I, dim)], 1)
    z = torch.einsum("bd,bcd->bc", q, V) * s
    loss = F.cross_entropy(z, torch.zeros(b, dtype=torch.long))
    (dloss * loss).backward()
    f = R.hardneg_fwd(q.detach(), p.detach(), n.detach(), s0, N, I, got_logits=z.detach())
    _close(f["logits"][0], z.detach(), "logits")
    _close(f["row_loss"][0].mean(), loss.detach(), "loss")
    dp0 = torch.randn(b, dim, dtype=torch.float64)
    o = R.hardneg_bwd(q.detach(), p.detach(), n.detach(), s0, z.detach(), f["lse"][0], dloss, N, I, dp0=dp0, dscale0=0.25)
    for k, want in (("dq", q.grad), ("dp", dp0 + p.grad), ("dn", n.grad), ("dscale", 0.25 + s.grad)):
        _close(o[k][0], want, k)


@pytest.mark.parametrize("temp", [None, 0.07])
def test_softce_reference_against_autograd(temp):
    sim, sim_m, ids_row, ids_all, _ = T.softce_inputs(257, seed=4)
    alpha, gscale, dloss = 0.4, 0.5, 0.37
    Tt = torch.tensor(1.0 if temp is None else float(np.float32(temp)), dtype=torch.float64, requires_grad=True)
    s = sim.double().requires_grad_(True)
    pos = (ids_all[None, :] == ids_row[:, None]).double()
    cnt = pos.sum(1, keepdim=True)
    hard = torch.where(cnt > 0, pos / cnt.clamp_min(1), torch.zeros_like(pos))
    a = float(np.float32(alpha))
    tgt = a * torch.softmax(sim_m.double() / Tt.detach(), 1) + (1 - a) * hard
    rl = -(torch.log_softmax(s / Tt, 1) * tgt).sum(1)
    o = R.softce(sim, sim_m, temp, ids_row, ids_all, alpha, gscale, dloss)
    _close(o["row_loss"][0], rl.detach(), "row_loss")
    gs = float(np.float32(gscale)) * float(np.float32(dloss))
    for i in range(sim.shape[0]):
        if i == 2:
            # no positive: the targets sum to alpha, not 1, and the header's g = softmax - target is no longer the derivative of the
            # row loss (the reference divides 0 / 0 there; a query's own id is always among ids_all).  The stated formula is kept.
            gi = (torch.softmax(s[i] / Tt, 0) - tgt[i]).detach() * gs
            _close(o["dsim"][0][i], gi / Tt.detach(), "dsim row 2")
            _close(o["row_dtemp"][0][i], -(gi * s[i].detach() / Tt.detach()).sum() / Tt.detach(), "dtemp row 2", rel=1e-11)
            continue
        ds, dT = torch.autograd.grad(gs * rl[i], (s, Tt), retain_graph=True)
        _close(o["dsim"][0][i], ds[i], f"dsim row {i}")
        _close(o["row_dtemp"][0][i], dT, f"dtemp row {i}", rel=1e-11)
    assert o["hit"][0][3:5].tolist() == [1.0, 0.0]


def test_normalize_reference_against_autograd():
    torch.manual_seed(5)
    emb = torch.randn(T.SELECT_SRC, 72, dtype=torch.float64, requires_grad=True)
    idx = T.select_idx()
    out = F.normalize(emb[idx.long()], dim=1)
    dout = torch.randn_like(out)
    (out * dout).sum().backward()
    f = R.select_normalize(emb.detach(), idx)
    _close(f["out"][0], out.detach(), "out")
    d0 = torch.randn(T.SELECT_SRC, 72, dtype=torch.float64)
    o = R.select_normalize_bwd(f["out"][0], f["inv_norm"][0], dout, idx, d0)
    _close(o["demb"][0], d0 + emb.grad, "demb")


# ================================================================================================================ the goldens
def test_references_against_golden_g1():
    d = np.load(os.path.join(GOLD, "g1_infonce_w1.npz"))
    for tag in ("a", "b"):
        t = lambda k: torch.tensor(d[f"{tag}_{k}"])          # noqa: E731
        emb = R.fuse_embeddings(t("txt"), t("img"), t("tmask"), t("imask"))["emb"][0]
        b = emb.shape[0] // 2
        iq = torch.arange(0, 2 * b, 2)
        q = R.select_normalize(emb, iq)["out"][0]
        p = R.select_normalize(emb, iq + 1)["out"][0]
        score = q @ p.t() * float(np.exp(np.log(1 / 0.07)))
        f = R.infonce_fwd(score, 0)
        assert float((score - torch.tensor(d[f"{tag}_score"]).double()).abs().max()) < 1e-3
        assert abs(float(f["loss"][0]) - float(d[f"{tag}_loss"])) < 1e-4
        assert float(f["acc"][0]) == float(d[f"{tag}_acc"])


@pytest.mark.parametrize("tag,ibn", [("n0", 0), ("n2", 2)])
def test_references_against_golden_g3(tag, ibn):
    d = np.load(os.path.join(GOLD, "g3_hardneg.npz"))
    emb = torch.tensor(d[f"{tag}_txt"] + d[f"{tag}_img"])
    b, N = 4, 2
    I = min(b - 1, ibn)
    iq = torch.arange(b) * 4
    ineg = (iq[:, None] + torch.tensor([2, 3])[None, :]).flatten()
    sel = {k: R.select_normalize(emb, i) for k, i in (("q", iq), ("p", iq + 1), ("n", ineg))}
    q, p, n = (sel[k]["out"][0] for k in "qpn")
    scale = 1 / 0.07
    f = R.hardneg_fwd(q, p, n, scale, N, I)
    z = f["logits"][0]
    f = R.hardneg_fwd(q, p, n, scale, N, I, got_logits=z)
    assert abs(float(f["row_loss"][0].mean()) - float(d[f"{tag}_loss"])) < 1e-5
    assert float(f["hit"][0].mean()) == float(d[f"{tag}_acc"])
    o = R.hardneg_bwd(q, p, n, scale, z, f["lse"][0], 1.0, N, I)
    demb = torch.zeros_like(emb, dtype=torch.float64)
    for k, i, grad in (("q", iq, o["dq"][0]), ("p", iq + 1, o["dp"][0]), ("n", ineg, o["dn"][0].reshape(b * N, -1))):
        demb = R.select_normalize_bwd(sel[k]["out"][0], sel[k]["inv_norm"][0], grad, i, demb)["demb"][0]
    assert float((demb - torch.tensor(d[f"{tag}_dtxt"]).double()).abs().max()) < 1e-5
    want = float(d[f"{tag}_dscale"])          # d loss / d logit_scale (the log-domain parameter)
    assert abs(float(o["dscale"][0]) * scale - want) < 1e-4 * max(1.0, abs(want))


# ================================================================================ fp32 restatements inside every bound, all cases
@pytest.mark.parametrize("c", T.NORM_FWD, ids=[c.name for c in T.NORM_FWD])
def test_norm_fwd_restatement_inside_bound(c):
    d = T.norm_inputs(c)
    ref = R.norm_fwd(d["x"], d["gamma"], d["beta"], c.eps, c.rms)
    got = norm_fwd32(d["x"], d["gamma"], d["beta"], np.float32(c.eps), c.rms)
    for k in got:
        _check("rms_fwd" if c.rms else "ln_fwd", got[k], ref[k], f"{c.name} {k}")


@pytest.mark.parametrize("c", T.NORM_BWD, ids=[c.name for c in T.NORM_BWD])
def test_norm_bwd_restatement_inside_bound(c):
    d = T.norm_inputs(c)
    ref = _norm_bwd_ref(c, d)
    got = norm_bwd32(c, d)
    assert set(got) == set(ref)
    for k in got:
        _check("rms_bwd" if c.rms else "ln_bwd", got[k], ref[k], f"{c.name} {k}")


def _norm_bwd_ref(c, d):
    return R.norm_bwd(d["x"], d["gamma"], d["dy"], c.eps, c.rms, dres=d.get("dres"), branch_scale=d.get("branch_scale"),
                      dgamma0=d["dgamma0"], dbeta0=d["dbeta0"], colsum0=d.get("colsum0"))


def test_sgemm_rules():
    """the chain is within the fp32 accumulation bound of the fp64 product; both accepted forms of an accumulating store are accepted,
    a neighbouring value and a chain with one k step missing are not; the split-K restatement differs from the chain within gamma"""
    rng = np.random.default_rng(0)
    A, B = rng.standard_normal((70, 400)).astype(np.float32), rng.standard_normal((400, 136)).astype(np.float32)
    acc = R.chain(A, B)
    ex = A.astype(np.float64) @ B.astype(np.float64)
    mag = np.abs(A).astype(np.float64) @ np.abs(B).astype(np.float64)
    assert (np.abs(acc - ex) <= R.gamma(400) * mag).all()
    sk = R.splitk_chain(A, B)
    assert (np.abs(sk - ex) <= R.gamma(400) * mag).all() and not np.array_equal(sk, acc)
    c0 = rng.standard_normal(acc.shape).astype(np.float32)
    for alpha in (np.float32(0.3), R.alpha32(1.7, 100.0)):
        two = (c0 + (acc * alpha).astype(np.float32)).astype(np.float32)
        fused = (acc.astype(np.float64) * np.float64(alpha) + c0.astype(np.float64)).astype(np.float32)
        assert (two != fused).any()
        for got in (two, fused):
            a, b = R.sgemm_accepts(got, acc, alpha, c0)
            assert (a | b).all()
        a, b = R.sgemm_accepts(np.nextafter(two, np.float32(np.inf)), acc, alpha, c0)
        assert not (a | b).all()
        a, _ = R.sgemm_accepts((acc * alpha).astype(np.float32), acc, alpha)
        assert a.all()
        a, _ = R.sgemm_accepts((R.chain(A[:, :-1], B[:-1]) * alpha).astype(np.float32), acc, alpha)
        assert not a.any()
    one, _ = R.sgemm_accepts((c0 + acc).astype(np.float32), acc, np.float32(1.0), c0)
    assert one.all()


@pytest.mark.parametrize("b,B,E,toff,scale", T.INFONCE)
def test_infonce_restatement_inside_bound(b, B, E, toff, scale):
    q, p = T.infonce_inputs(b, B, E)
    z = torch.from_numpy((R.chain(q.numpy(), p.numpy().T) * R.alpha32(1.0, scale)).astype(np.float32))
    ref = R.infonce_fwd(z, toff)
    got = infonce_fwd32(z, toff)
    for k in got:
        _check("infonce_fwd", got[k], ref[k], f"infonce {b}x{B} {k}")
    refb = R.infonce_bwd(q, p, np.float32(scale), z, got["lse"], np.float32(T.DLOSS), toff)
    gotb = infonce_bwd32(q, p, scale, z, got["lse"], T.DLOSS, toff)
    for k in gotb:
        _check("infonce_bwd", gotb[k], refb[k], f"infonce {b}x{B} {k}")


@pytest.mark.parametrize("delta,where", T.TIES)
def test_infonce_ties_reference(delta, where):
    q, p, toff, want = T.tie_inputs(delta, where)
    z = torch.from_numpy(R.chain(q.numpy(), p.numpy().T))
    assert int((z == z.max()).sum()) == 2, "the two equal maxima"
    assert float(R.infonce_fwd(z, toff)["hit"][0]) == want


@pytest.mark.parametrize("b,N,I,dim", T.HARDNEG)
def test_hardneg_restatement_inside_bound(b, N, I, dim):
    q, p, n = T.hardneg_inputs(b, N, I, dim)
    dp0, ds0, scale = torch.randn(b, dim), 0.25, 14.0
    fwd, bwd = hardneg32(q, p, n, scale, N, I, T.DLOSS, dp0, ds0)
    ref = R.hardneg_fwd(q, p, n, scale, N, I, got_logits=fwd["logits"])
    for k in fwd:
        _check("hardneg_fwd", fwd[k], ref[k], f"hardneg {k}")
    refb = R.hardneg_bwd(q, p, n, scale, fwd["logits"], fwd["lse"], np.float32(T.DLOSS), N, I, dp0=dp0, dscale0=ds0)
    assert set(bwd) == set(refb)
    for k in bwd:
        _check("hardneg_bwd", bwd[k], refb[k], f"hardneg {k}")
    if N and b >= 2:
        assert fwd["hit"][0] == 0.0 and fwd["hit"][1] == 1.0 and float(fwd["logits"][1, 0]) == float(fwd["logits"][1, 1])


@pytest.mark.parametrize("n,temp,alpha", T.SOFTCE)
def test_softce_restatement_inside_bound(n, temp, alpha):
    sim, sim_m, ids_row, ids_all, hits = T.softce_inputs(n)
    ref = R.softce(sim, sim_m, temp, ids_row, ids_all, alpha, 0.5, T.DLOSS)
    got = softce32(sim, sim_m, temp, ids_row, ids_all, alpha, 0.5, T.DLOSS)
    for k in got:
        _check("softce", got[k], ref[k], f"softce n={n} {k}")
    for row, want in hits.items():
        assert float(ref["hit"][0][row]) == want
    assert int((ids_all == ids_row[1]).sum()) == 3 and int((ids_all == ids_row[2]).sum()) == 0


@pytest.mark.parametrize("dim", T.SELECT_DIMS)
def test_select_restatements_inside_bound(dim):
    torch.manual_seed(dim)
    emb = torch.randn(T.SELECT_SRC, dim)
    for idx in (T.select_idx(), None):
        src = emb if idx is not None else emb[:T.SELECT_SRC - 1]
        x = src[idx.long()] if idx is not None else src
        nrm = torch.sqrt(s32(x * x))[:, None].clamp_min(1e-12)
        ref = R.select_normalize(src, idx)
        _check("select_normalize", x / nrm, ref["out"], "out")
        _check("select_normalize", (1.0 / nrm)[:, 0], ref["inv_norm"], "inv_norm")
        out, inv = (x / nrm), (1.0 / nrm)[:, 0]
        dout, d0 = torch.randn_like(out), torch.randn_like(src)
        _check("select_normalize_bwd", select_bwd32(out, inv, dout, idx, d0)["demb"],
               R.select_normalize_bwd(out, inv, dout, idx, d0)["demb"], "demb")


@pytest.mark.parametrize("dim", T.FUSE_DIMS)
def test_fuse_restatement_inside_bound(dim):
    txt, img, tm, im, demb = T.fuse_inputs(dim)
    _check("fuse", txt * tm[:, None] + img * im[:, None], R.fuse_embeddings(txt, img, tm, im)["emb"], "emb")
    ref = R.fuse_embeddings_bwd(demb, tm, im)
    _check("fuse_bwd", demb * tm[:, None], ref["dtxt"], "dtxt")
    _check("fuse_bwd", demb * im[:, None], ref["dimg"], "dimg")


@pytest.mark.parametrize("n,Tk,W", T.MEANPOOL)
def test_meanpool_restatement_inside_bound(n, Tk, W):
    torch.manual_seed(W)
    x = torch.randn(n, Tk, W)
    _check("meanpool", s32(x, 1) / Tk, R.meanpool_fwd(x)["out"], "out")
    d = torch.randn(n, W)
    _check("meanpool", (d * np.float32(1.0 / Tk))[:, None, :].expand(n, Tk, W), R.meanpool_bwd(d, Tk)["dx"], "dx")


@pytest.mark.parametrize("count", T.ADAMW_COUNTS + (T.ADAMW_BIG,))
def test_adamw_restatement_inside_bound(count):
    """the GPU test's plan, step by step from the state the step before left"""
    p, g, m, v = T.adamw_inputs(count)
    for step, wd, gs, _ in (T.ADAMW_BIG_PLAN if count == T.ADAMW_BIG else T.ADAMW_PLAN):
        ref = R.adamw_step(p, g, m, v, wd=wd, step=step, grad_scale=gs, **T.ADAM)
        got = adamw32(p, g, m, v, wd=wd, step=step, gs=gs, **T.ADAM)
        for k in got:
            _check("adamw", got[k], ref[k], f"adamw {k} step {step}")
        p, m, v = got["param"], got["exp_avg"], got["exp_avg_sq"]


def test_ema_restatement_inside_bound():
    pm, p, _, _ = T.adamw_inputs(T.EMA_COUNT, seed=3)
    mo = np.float32(T.EMA_MOMENTUM)
    _check("ema", pm * mo + p * (np.float32(1) - mo), R.ema_update(pm, p, T.EMA_MOMENTUM)["param_m"], "ema")


def test_ratio_table_of_the_restatements():
    """every restatement test once more, in this test alone, for the table of the worst |got - ref| / bound per operation (each
    check asserts its own ratio <= 0.5; the table does not depend on which other tests ran)"""
    RATIOS.clear()
    for c in T.NORM_FWD:
        test_norm_fwd_restatement_inside_bound(c)
    for c in T.NORM_BWD:
        test_norm_bwd_restatement_inside_bound(c)
    for a in T.INFONCE:
        test_infonce_restatement_inside_bound(*a)
    for a in T.HARDNEG:
        test_hardneg_restatement_inside_bound(*a)
    for a in T.SOFTCE:
        test_softce_restatement_inside_bound(*a)
    for d in T.SELECT_DIMS:
        test_select_restatements_inside_bound(d)
    for d in T.FUSE_DIMS:
        test_fuse_restatement_inside_bound(d)
    for a in T.MEANPOOL:
        test_meanpool_restatement_inside_bound(*a)
    for n in T.ADAMW_COUNTS:
        test_adamw_restatement_inside_bound(n)
    test_ema_restatement_inside_bound()
    ops = {"ln_fwd", "rms_fwd", "ln_bwd", "rms_bwd", "infonce_fwd", "infonce_bwd", "hardneg_fwd", "hardneg_bwd", "softce",
           "select_normalize", "select_normalize_bwd", "fuse", "fuse_bwd", "meanpool", "adamw", "ema"}
    assert set(RATIOS) == ops, set(RATIOS) ^ ops
    for op, r in sorted(RATIOS.items()):
        print(f"OBS cpu fp32 restatement {op:22s} worst |got - ref| / bound = {r:.3f}")
    assert all(r <= 0.5 for r in RATIOS.values()), dict(RATIOS)


# ============================================================================================================ planted defects
def _violates(got, ref_bound):
    ref, bound = ref_bound
    return bool(R.violations(got, ref, bound).any())


def _case(table, name):
    return next(c for c in table if c.name == name)


@pytest.mark.parametrize("defect", ["drop_column", "padded_mean"])
def test_planted_ln_fwd_defects_violate(defect):
    c = _case(T.NORM_FWD, "ln-fwd-w260")
    d = T.norm_inputs(c)
    ref = R.norm_fwd(d["x"], d["gamma"], d["beta"], c.eps, False)
    got = norm_fwd32(d["x"], d["gamma"], d["beta"], np.float32(c.eps), False, defect)
    assert _violates(got["y_f32"], ref["y_f32"]) and _violates(got["y_bf16"], ref["y_bf16"])
    with pytest.raises(AssertionError):
        R.check(got["y_f32"], *ref["y_f32"], defect)


def test_planted_rms_beta_violates():
    c = _case(T.NORM_FWD, "rms-fwd-w764")
    d = T.norm_inputs(c)
    ref = R.norm_fwd(d["x"], d["gamma"], d["beta"], c.eps, True)
    got = norm_fwd32(d["x"], d["gamma"], d["beta"], np.float32(c.eps), True, "rms_beta")
    assert _violates(got["y_f32"], ref["y_f32"]) and _violates(got["y_bf16"], ref["y_bf16"])


@pytest.mark.parametrize("defect,key", [("dres_stride", "dx_f32"), ("scale_dx_f32", "dx_f32"), ("dgamma_overwrite", "dgamma")])
def test_planted_ln_bwd_defects_violate(defect, key):
    c = _case(T.NORM_BWD, "ln-bwd-w764-f32-opts")
    d = T.norm_inputs(c)
    ref = _norm_bwd_ref(c, d)
    assert not _violates(norm_bwd32(c, d)[key], ref[key])
    assert _violates(norm_bwd32(c, d, defect)[key], ref[key])


@pytest.mark.parametrize("defect,key", [("argmax_last", "hit"), ("target_off", "row_loss")])
def test_planted_infonce_defects_violate(defect, key):
    q, p, toff, _ = T.tie_inputs(70, "first")
    z = torch.from_numpy(R.chain(q.numpy(), p.numpy().T))
    ref = R.infonce_fwd(z, toff)
    assert not _violates(infonce_fwd32(z, toff)[key], ref[key])
    assert _violates(infonce_fwd32(z, toff, defect)[key], ref[key])


def test_planted_softce_inv_pos_violates():
    sim, sim_m, ids_row, ids_all, _ = T.softce_inputs(257)
    ref = R.softce(sim, sim_m, 0.07, ids_row, ids_all, 0.4, 0.5, None)
    got = softce32(sim, sim_m, 0.07, ids_row, ids_all, 0.4, 0.5, None, "inv_pos_n")
    assert _violates(got["row_loss"], ref["row_loss"]) and _violates(got["dsim"], ref["dsim"])


def test_planted_duplicate_destination_violates():
    torch.manual_seed(0)
    idx = T.select_idx()
    out = F.normalize(torch.randn(T.SELECT_ROWS, 72), dim=1)
    inv, dout, d0 = torch.rand(T.SELECT_ROWS) + 0.5, torch.randn(T.SELECT_ROWS, 72), torch.randn(T.SELECT_SRC, 72)
    ref = R.select_normalize_bwd(out, inv, dout, idx, d0)["demb"]
    assert not _violates(select_bwd32(out, inv, dout, idx, d0)["demb"], ref)
    bad = R.violations(select_bwd32(out, inv, dout, idx, d0, "dup_once")["demb"], *ref)
    assert bad[5].any() and not bad[30:].any()          # the repeated destination is caught, the unselected rows are exact


def test_planted_adamw_bias_step_violates():
    p, g, m, v = T.adamw_inputs(1003)
    ref = R.adamw_step(p, g, m, v, wd=0.2, step=3, grad_scale=0.5, **T.ADAM)
    assert not _violates(adamw32(p, g, m, v, wd=0.2, step=3, gs=0.5, **T.ADAM)["param"], ref["param"])
    assert _violates(adamw32(p, g, m, v, wd=0.2, step=3, gs=0.5, defect="bias_step", **T.ADAM)["param"], ref["param"])


def test_one_lost_row_of_the_long_case_violates_dbeta():
    """the 8231-row cases: integer dy makes dbeta exact, so a single row missing from the column sums is caught (the bounds of
    dgamma and dx_colsum are wider than one row's term at that many rows)"""
    c = _case(T.NORM_BWD, "ln-bwd-long-pred")
    d = T.norm_inputs(c)
    ref = _norm_bwd_ref(c, d)
    assert float(ref["dbeta"][1].max()) == 0.0
    got = norm_bwd32(c, d)["dbeta"]
    assert not _violates(got, ref["dbeta"])
    lost = got - d["dy"][5000].float()          # a row of the loop's second pass
    assert R.violations(lost, *ref["dbeta"]).sum() == (d["dy"][5000] != 0).sum()


def test_nan_and_inf_are_violations():
    ref, bound = torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64)
    got = torch.tensor([0.0, float("nan"), float("inf"), 0.5])
    assert R.violations(got, ref, bound).tolist() == [False, True, True, False]
    assert R.worst_ratio(got, ref, bound) == float("inf")


# ============================================================================================================= host arithmetic
def test_norm_cases_name_their_kernel_instance():
    for w, path in T.FWD_WIDTHS.items():
        nc, exact = R.ln_path(w)
        assert f"NC{nc}{'e' if exact else 'p'}" == path, w
    for w, path in T.GRID_WIDTHS.items():
        assert T.FWD_WIDTHS[w] == path
    assert {c.path for c in T.NORM_FWD if not c.rms} == {f"NC{n}{e}" for n in (2, 3, 4, 8) for e in "ep"}
    assert {c.path for c in T.NORM_FWD if c.rms} == {f"NC{n}{e}" for n in (2, 3, 4, 8) for e in "ep"}
    for rms in (False, True):
        inst = {(c.path, c.dy_f32) for c in T.NORM_BWD if c.rms == rms}
        assert inst == {(f"NC{n}{e}", f) for n in (2, 3, 4, 8) for e in "ep" for f in (False, True)}
    # every (LayerNorm instance, option value) pair
    pairs = {(c.path, c.dy_f32, c.opts) for c in T.NORM_BWD if not c.rms}
    assert len(pairs) == 32
    # lane 0 alone owns a chunk of the second pass at 260; 8231 rows exceed any resident grid (8 x 256 workgroups x 4 rows)
    assert 260 // 4 == 65 and T.LONG_ROWS > 8 * 256 * 4
    for c in T.NORM_BWD:
        assert (c.workgroups == 1) == (c.rows <= 4)


def test_sgemm_cases_name_their_kernel():
    for c in T.SGEMM + list(T.BOUNDARY):
        assert c.expected_path() == c.path, (c.name, c.expected_path())
    assert {c.path for c in T.SGEMM} == {"S1", "S2", "S3", "S4", "S5", "S6"}
    assert T.BOUNDARY[0].M * T.BOUNDARY[0].N == 128 * 128 * 8
    assert R.splitk_plan(132, 136, 400) == (3, 144, 3)
    assert R.splitk_plan(132, 136, 1296) == (10, 144, 9)          # the workspace is sized by 10 slices, 9 run
    assert R.splitk_plan(256, 768, 57344)[0] == 86
    for (b, B, E, toff, _) in T.INFONCE:
        assert T.infonce_launch_paths(b, B, E) == T.INFONCE_PATHS[(b, B, E, toff)]
    assert T.HARDNEG[-1][1] + T.HARDNEG[-1][2] + 1 > 256
    assert T.ADAMW_BIG == 16_777_221 and -(-(T.ADAMW_BIG // 4 + 1) // 256) > 16384
