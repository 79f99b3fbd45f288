"""Every gradient sum that used to land in arrival order now has one fixed order: the T5 relative-position-bias gradient
(uniir_attention_rel_bwd), the hard-negative loss's d scale (uniir_hardneg_bwd), the scatter of uniir_select_normalize_bwd with repeated
destinations, and token buckets longer than the LDS sort of uniir_text_embed_bwd{,_packed}.  "Repeat" below: REPEAT runs on identical
inputs, every result torch.equal to the first, non-zero, and inside a bound of an fp64 reference.  Then two whole training steps
(CLIP_FF, CLIP_SF with hard negatives) bit for bit, and the lapse counter: a reduction whose stream has too small a scratch buffer
keeps its atomics, uniir_reduce_stats says so, and uniir_amd.ops grows the buffer.

Bounds.  The rel-bias gradient is held to the drel bound of tests/test_attention_paths_gpu.py (its _drel, on the fp64 reference of
tests/attention_ref.py).  The fp32 kernels are held to 1e-5 of the largest reference element (G3's gate): an fp32 sum of n <= 6000
terms of one magnitude in chunks of <= 1024 carries about 2^-24 * sqrt(n^2 / 2) of a term, a few 1e-5 of a TERM, while the largest sums
are tens of terms, so correct arithmetic sits one to two orders below the gate."""
import ctypes as C
import os
import sys
import warnings
from types import SimpleNamespace

import pytest
import torch

import attention_ref as R
import test_attention_paths_gpu as P          # its guarded buffers + calls (Run) and its drel bound (_drel), used as they are

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))
DEV = "cuda"
REPEAT = 8
GATE = 1e-5


def _relmax(got, ref):
    return float((got.double() - ref).abs().max() / ref.abs().max())


def _repeat(fn):
    """fn() -> dict of tensors, REPEAT times; every run equal to the first, nothing all-zero -> the first"""
    first = {k: v.clone() for k, v in fn().items()}
    torch.cuda.synchronize()
    for k, v in first.items():
        assert float(v.abs().max()) > 0, f"{k} is all zero"
    for i in range(1, REPEAT):
        for k, v in fn().items():
            assert torch.equal(v, first[k]), f"{k}: run {i} differs from run 0 by up to {float((v - first[k]).abs().max()):.3g}"
    return first


# ---- 1. relative-position-bias gradient ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seq,batch,drop_p", [(80, 48, 0.0), (80, 48, 0.1), (334, 48, 0.0), (334, 48, 0.1), (512, 2, 0.0)],
                         ids=lambda v: str(v))
def test_rel_bias_gradient_repeats_bit_for_bit(seq, batch, drop_p):
    """48 x 4 workgroups into 32 x 4 floats with CLIP_FF's bucket table: 80 tokens (five key tiles: several waves feed one diagonal)
    and 334 (CLIP_FF's own length); 512 tokens x 2 items for the LDS budget of the 64-bit diagonal sums"""
    from uniir_amd import clipff_model, ops
    heads, nb = 4, clipff_model.T5_BUCKETS
    assert nb == 32
    c = R.Case(f"repro-rel-{seq}-{drop_p}", "attn_bwd_kernel<rel>", "rel", batch, heads, seq, drop_p=drop_p, nbuckets=nb, seed=seq)
    items = R.build_items(c, DEV, P._dropf(drop_p) if drop_p > 0 else None)
    table = clipff_model.rel_bucket_table(seq).to(DEV)
    assert table.numel() == 2 * seq - 1 and 0 <= int(table.min()) and int(table.max()) < nb
    for it in items:
        it.rel_bucket = table
    run = P.Run(c, items)
    run.forward()
    out_in, lse_in = P._round_ref(c, [it.fwd_ref()[0] for it in items])
    ops.reset_reduce_stats()
    run.backward(out_in, lse_in)
    refs, _ = P._bwd_refs(items, out_in, lse_in)
    ratios = {}
    first = P._drel(c, run, refs, ratios, "backward")          # asserts the bound of test_attention_paths_gpu on the same quantity
    dx = run.dX.bits().clone()
    print(f"\nOBS {c.name} drel worst |got - ref| / bound = {ratios['drel']:.3f}, max |drel| = {float(first.abs().max()):.4g}")
    assert float(first.abs().max()) > 0
    for i in range(1, REPEAT):
        run.backward(out_in, lse_in)
        again = run.drel.view[0].view(nb, heads)
        assert torch.equal(again, first), f"drel: run {i} differs from run 0 by up to {float((again - first).abs().max()):.3g}"
        assert torch.equal(run.dX.bits(), dx), f"dqkv: run {i} differs from run 0"
    assert ops.reduce_stats()[0] == 0


# ---- 2. hard-negative loss -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [0, 3])
def test_hardneg_bwd_repeats_bit_for_bit(I):
    """b = 300 query blocks used to race into the one float of dscale.  N = 2 negatives, dim 64.  The data is chosen so that the
    gate measures the kernel and not the conditioning of the inputs: d scale = (g / s) sum_i sum_n p_n (l_n - l_0), which the kernel
    (like autograd) evaluates as sum_c (p_c - [c = 0]) l_c.  With negatives that really are hard (cosine 0.6 to the query, the
    positive 0.29) every row has l_n > l_0, so all rows pull d scale the same way and the sum of the absolute terms is 2.7 times the
    result for I = 0 and I = 3 alike; with easy negatives that ratio was 14 000 at I = 3 and fp32 torch itself missed the gate by ten
    times.  Nor is any output a difference of nearly equal numbers (a positive's probability within 1e-4 of 1 leaves the factor
    p - 1 of dq known to 1e-3 in any fp32 arithmetic)."""
    from uniir_amd import ops
    b, N, E = 300, 2, 64
    g = torch.Generator().manual_seed(31 + I)
    nrm = torch.nn.functional.normalize
    q = nrm(torch.randn(b, E, generator=g), dim=-1)
    p = nrm(0.3 * q + nrm(torch.randn(b, E, generator=g), dim=-1), dim=-1)
    n = nrm(0.75 * q.repeat_interleave(N, 0) + nrm(torch.randn(b * N, E, generator=g), dim=-1), dim=-1)
    scale, dloss = torch.tensor([14.0]), torch.tensor([1.7])
    # fp64 reference (the logit row of clip_sf.py:105-131 as include/uniir_hip.h states it)
    q64, p64, n64, s64 = (t.double().to(DEV).requires_grad_(True) for t in (q, p, n, scale))
    pos = (q64 * p64).sum(-1, keepdim=True)
    row = torch.cat([pos, torch.einsum("be,bne->bn", q64, n64.view(b, N, E))] + [pos] * I, dim=1) * s64
    loss = (torch.logsumexp(row, -1) - row[:, 0]).mean()
    (loss * dloss.double().to(DEV)).sum().backward()
    ref = dict(dq=q64.grad, dp=p64.grad, dn=n64.grad, dscale=s64.grad)
    qd, pd, nd, sd, dl = (t.to(DEV).contiguous() for t in (q, p, n, scale, dloss))
    Cn = 1 + N + I
    logits, lse = torch.empty(b, Cn, device=DEV), torch.empty(b, device=DEV)
    ops.call("uniir_hardneg_fwd", qd, pd, nd, sd, b, N, I, E, logits, lse, torch.empty(b, device=DEV), torch.empty(b, device=DEV))

    def bwd():
        dq, dn = torch.empty(b, E, device=DEV), torch.empty(b * N, E, device=DEV)
        dp, dscale = torch.zeros(b, E, device=DEV), torch.zeros(1, device=DEV)
        ops.call("uniir_hardneg_bwd", qd, pd, nd, sd, logits, lse, dl, b, N, I, E, dq, dp, dn, dscale)
        return dict(dq=dq, dp=dp, dn=dn, dscale=dscale)
    got = _repeat(bwd)
    for k, v in got.items():
        r = _relmax(v, ref[k])
        print(f"OBS hardneg I={I} {k} relative error {r:.3g}")
        assert r < GATE, (k, r)


@pytest.mark.parametrize("with_idx", [True, False])
def test_select_normalize_bwd_repeats_bit_for_bit(with_idx):
    """2048 rows of dim 512 scattered to 8 destinations (256 adds each, destinations 3, 5, .. of a 24-row table); and idx = None"""
    from uniir_amd import ops
    rows, E, M = 2048, 512, 24
    g = torch.Generator().manual_seed(41)
    x = torch.randn(rows, E, generator=g)
    inv = (1.0 / x.norm(dim=-1)).to(DEV)
    y = torch.nn.functional.normalize(x, dim=-1).to(DEV)
    dy = torch.randn(rows, E, generator=g).to(DEV)
    idx = (3 + 2 * torch.randint(0, 8, (rows,), generator=g)).to(torch.int32).to(DEV) if with_idx else None
    contrib = (dy.double() - y.double() * (y.double() * dy.double()).sum(-1, keepdim=True)) * inv.double()[:, None]
    if with_idx:
        assert sorted(set(idx.tolist())) == [3, 5, 7, 9, 11, 13, 15, 17]
        ref = torch.zeros(M, E, dtype=torch.float64, device=DEV).index_add_(0, idx.long(), contrib)
    else:
        ref = contrib

    def bwd():
        demb = torch.zeros(M if with_idx else rows, E, device=DEV)
        ops.call("uniir_select_normalize_bwd", y, inv, dy, idx, demb, rows, E)
        return dict(demb=demb)
    got = _repeat(bwd)["demb"]
    if with_idx:
        assert not bool(got[0::2].any()) and not bool(got[19:].any())          # rows nobody selected stay zero
    r = _relmax(got, ref)
    print(f"OBS select_normalize_bwd idx={with_idx} relative error {r:.3g}")
    assert r < GATE, r


# ---- 3. token buckets longer than the LDS sort, with gradients that are not zero ---------------------------------------------------
def _token_case(n, ctx, vocab, wdt, ids, seed):
    from uniir_amd import ops
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(60, ctx + 1, (n,), generator=g)
    live = (torch.arange(ctx).unsqueeze(0) < lens.unsqueeze(1)).flatten()
    dx = torch.randn(n * ctx, wdt, generator=g).to(DEV)
    idd = ids.to(torch.int32).to(DEV).contiguous()
    row_off = torch.zeros(n + 1, dtype=torch.int32)
    row_off[1:] = torch.cumsum(lens, 0)
    ro, dxp = row_off.to(DEV), dx[live.to(DEV)].contiguous()
    flat = idd.flatten().long()

    def dense():
        dt, dp = torch.zeros(vocab, wdt, device=DEV), torch.zeros(ctx, wdt, device=DEV)
        ops.call("uniir_text_embed_bwd", idd, dx, dt, dp, n, ctx, wdt, vocab)
        return dict(dtok=dt, dpos=dp)

    def packed():
        dt, dp = torch.zeros(vocab, wdt, device=DEV), torch.zeros(ctx, wdt, device=DEV)
        ops.call("uniir_text_embed_bwd_packed", idd, dxp, ro, dt, dp, n, ctx, wdt, vocab)
        return dict(dtok=dt, dpos=dp)
    ref_d = torch.zeros(vocab, wdt, dtype=torch.float64, device=DEV).index_add_(0, flat, dx.double())
    ref_p = torch.zeros(vocab, wdt, dtype=torch.float64, device=DEV).index_add_(0, flat[live.to(DEV)], dxp.double())
    return dense, packed, ref_d, ref_p, live


def test_long_token_bucket_with_nonzero_gradients_repeats_bit_for_bit():
    """96 captions x 77 positions = 7392 rows (two row slices of 4096), vocabulary 512, width 320 (a full and a partial column slab).
    About 6000 rows share id 7 and carry random gradients -- a bucket longer than the LDS sort, filled by integer atomics in
    arrival order -- and the rest collide among the 64 ids 100 .. 163.  Dense and packed (row_off) forms."""
    from uniir_amd import ops
    n, ctx, vocab, wdt = 96, 77, 512, 320
    g = torch.Generator().manual_seed(51)
    ids = torch.where(torch.rand(n, ctx, generator=g) < 0.81, torch.full((n, ctx), 7), torch.randint(100, 164, (n, ctx), generator=g))
    dense, packed, ref_d, ref_p, live = _token_case(n, ctx, vocab, wdt, ids, 52)
    assert int((ids == 7).sum()) > 5500 and int(((ids == 7).flatten() & live).sum()) > 4096          # long in both forms
    ops.reset_reduce_stats()
    for name, fn, ref in (("dense", dense, ref_d), ("packed", packed, ref_p)):
        got = _repeat(fn)["dtok"]
        r = _relmax(got, ref)
        print(f"OBS text_embed_bwd {name} long bucket relative error {r:.3g}")
        assert r < GATE, (name, r)
        assert not bool(got[:7].any()) and not bool(got[164:].any())
    assert ops.reduce_stats()[0] == 0


def test_more_long_token_buckets_than_one_round_takes():
    """nine ids of 4106 .. 4107 rows each (36960 rows, ten row slices): the long ids are taken eight at a time, so the ninth goes
    through a second round of the slice kernels"""
    n, ctx, vocab, wdt = 480, 77, 64, 8
    ids = (torch.arange(n * ctx) % 9 + 20).view(n, ctx)
    dense, packed, ref_d, ref_p, live = _token_case(n, ctx, vocab, wdt, ids, 53)
    assert int((ids == 28).sum()) > 4096
    got = _repeat(dense)["dtok"]
    assert _relmax(got, ref_d) < GATE, _relmax(got, ref_d)
    assert not bool(got[:20].any()) and not bool(got[29:].any()) and all(float(got[i].abs().max()) > 0 for i in range(20, 29))
    gp = _repeat(packed)["dtok"]
    assert _relmax(gp, ref_p) < GATE, _relmax(gp, ref_p)


# ---- 4. whole steps ------------------------------------------------------------------------------------------------------------------
T5 = dict(d_model=128, num_heads=2, d_ff=256, num_layers=2)


def _clipff_step(cfg, dbatch):
    """a freshly built tiny CLIP_FF (the configuration of tests/test_recompute_towers_gpu.py), one forward + backward"""
    from oracle import clip_oracle as O
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from uniir_amd import clip_model
    clip_model.CLIP_CONFIGS["tiny-ff-repro"] = cfg
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    m = CLIPFeatureFusion("tiny-ff-repro", device="cuda", config=config, t5_config=dict(T5, dropout_rate=0.0))
    sd = O.init_state_dict(cfg, seed=5)
    sd.pop("text_projection")
    m.clip_model.load_state_dict(sd, strict=True)
    clip = m.clip_model
    m.train()
    clip._ensure_flat()
    m._ensure_t5()
    m.zero_grad()
    out = m(dbatch)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {"clip." + n: p.grad.detach().clone() for n, p in clip.named_parameters() if p.grad is not None}
    grads.update({"t5." + n: p.grad.detach().clone() for n, p in m.t5_layers.named_parameters() if p.grad is not None})
    return out["loss"].detach().clone(), grads


def test_clipff_step_is_reproducible_for_every_parameter():
    """two freshly built models, same seed and batch (4 pairs, dropout 0): every parameter gradient bit for bit, the T5
    relative-position bias included; no reduction of the step fell back to atomics"""
    from oracle import clip_oracle as O
    from uniir_amd import ops
    cfg = O.tiny_config(vision_width=128, vision_layers=3, transformer_width=128, transformer_heads=2, transformer_layers=3, embed_dim=128)
    batch = O.synthetic_batch(cfg, 4, seed=23)
    dbatch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    ops.reset_reduce_stats()
    loss_a, a = _clipff_step(cfg, dbatch)
    loss_b, b = _clipff_step(cfg, dbatch)
    assert ops.reduce_stats()[0] == 0, ops.reduce_stats()
    assert torch.equal(loss_a, loss_b)
    assert set(a) == set(b) and len(a) > 80
    rel = [n for n in a if n.endswith("SelfAttention.relative_attention_bias.weight")]
    assert len(rel) == 1 and float(a[rel[0]].abs().max()) > 0
    for n, g in a.items():
        assert torch.equal(b[n], g), (n, float((b[n] - g).abs().max()), float(g.abs().max()))


def test_clipsf_hard_negative_step_is_reproducible():
    """tiny CLIP_SF, the hard-negative branch on: 4 queries x 2 hard negatives, in_batch_neg_num 2, and one candidate that is a
    negative of two queries (two source rows for one row of the embedding gradient).  The whole flat gradient bit for bit."""
    from oracle import clip_oracle as O
    from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
    from uniir_amd import clip_model, ops
    cfg = O.tiny_config()
    clip_model.CLIP_CONFIGS["tiny-sf-repro"] = cfg
    b, nneg = 4, 2
    flat = O.synthetic_batch(cfg, b * (2 + nneg) // 2, seed=19)
    im = {"query": [], "pos_cand": [], "neg_cand_list": []}
    c = 0
    for _ in range(b):
        im["query"].append([c]); c += 1
        im["pos_cand"].append([c]); c += 1
        im["neg_cand_list"].append(list(range(c, c + nneg))); c += nneg
    im["neg_cand_list"][1][0] = im["neg_cand_list"][0][1]          # item 3: a negative of query 0 and of query 1
    flat["index_mapping"] = im
    dbatch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in flat.items()}
    ops.reset_reduce_stats()

    def step():
        config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=2))
        model = CLIPScoreFusion("tiny-sf-repro", device="cuda", config=config)
        model.clip_model.load_state_dict(O.init_state_dict(cfg, seed=3), strict=True)
        model.in_batch_neg_num = 2
        model.train()
        model.clip_model._ensure_flat()
        model.clip_model.zero_grad()
        out = model(dbatch)
        out["loss"].backward()
        torch.cuda.synchronize()
        return out["loss"].detach().clone(), model.clip_model._flat["g32"].clone(), model.clip_model.logit_scale.grad.clone()
    la, ga, sa = step()
    lb, gb, sb = step()
    assert ops.reduce_stats()[0] == 0, ops.reduce_stats()
    assert float(ga.abs().max()) > 0 and float(sa.abs()) > 0
    assert torch.equal(la, lb) and torch.equal(sa, sb)
    assert torch.equal(ga, gb), (int((ga != gb).sum()), float((ga - gb).abs().max()))


# ---- 5. the lapse is visible, and the host side repairs it -----------------------------------------------------------------------
LN_ROWS, LN_WIDTH = 20000, 256


def _ln_case():
    g = torch.Generator().manual_seed(61)
    x, gamma = torch.randn(LN_ROWS, LN_WIDTH, generator=g).to(DEV), (1.0 + 0.1 * torch.randn(LN_WIDTH, generator=g)).to(DEV)
    dy = torch.randn(LN_ROWS, LN_WIDTH, generator=g).to(DEV)
    xr, gr = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    br = torch.zeros(LN_WIDTH, device=DEV, requires_grad=True)
    torch.nn.functional.layer_norm(xr, (LN_WIDTH,), gr, br, 1e-5).backward(dy)
    return x, gamma, dy, dict(dx=xr.grad, dgamma=gr.grad, dbeta=br.grad)


def test_a_reduction_without_enough_scratch_is_counted():
    """a fresh stream with a 4 KiB scratch registered through the C ABI; uniir_layernorm_bwd at 20000 x 256 asks for g * 3 * 256 * 4
    bytes (g = its persistent workgroups: at least one per compute unit, at most rows / 4), gets none, keeps its atomics and is counted;
    the result is still right"""
    from uniir_amd import _lib, ops
    lib = _lib.load()
    x, gamma, dy, ref = _ln_case()
    s = torch.cuda.Stream()
    small = torch.empty(4096, dtype=torch.uint8, device=DEV)
    handle = C.c_void_p(s.cuda_stream)
    _lib.check(lib.uniir_reduce_scratch(C.c_void_p(small.data_ptr()), 4096, handle), "reduce_scratch")
    try:
        torch.cuda.synchronize()
        ops.reset_reduce_stats()
        f0, _ = ops.reduce_stats()
        dx = torch.empty(LN_ROWS, LN_WIDTH, device=DEV)
        dg, db = torch.zeros(LN_WIDTH, device=DEV), torch.zeros(LN_WIDTH, device=DEV)
        with torch.cuda.stream(s):
            _lib.check(lib.uniir_layernorm_bwd(x.data_ptr(), LN_WIDTH, gamma.data_ptr(), dy.data_ptr(), 1, None, dx.data_ptr(), LN_WIDTH,
                                               None, dg.data_ptr(), db.data_ptr(), None, LN_ROWS, LN_WIDTH, 1e-5, handle), "ln_bwd")
        s.synchronize()
        f1, mreq = ops.reduce_stats()
        assert f1 >= f0 + 1, (f0, f1)
        # the request is g * 3 * width * 4 bytes with g = min(rows / 4, workgroups per compute unit x 256 compute units)
        per_wg = 3 * LN_WIDTH * 4
        g = mreq // per_wg
        assert mreq == g * per_wg and (g == LN_ROWS // 4 or (g % 256 == 0 and 256 <= g < LN_ROWS // 4)), (mreq, g)
        # ... and it is what the launch really needs: one byte less is a lapse again, exactly that much is not
        exact = torch.empty(mreq, dtype=torch.uint8, device=DEV)
        for nbytes, lapses in ((mreq - 1, 1), (mreq, 0)):
            _lib.check(lib.uniir_reduce_scratch(C.c_void_p(exact.data_ptr()), nbytes, handle), "reduce_scratch")
            before = ops.reduce_stats()[0]
            dg2, db2 = torch.zeros(LN_WIDTH, device=DEV), torch.zeros(LN_WIDTH, device=DEV)
            with torch.cuda.stream(s):
                _lib.check(lib.uniir_layernorm_bwd(x.data_ptr(), LN_WIDTH, gamma.data_ptr(), dy.data_ptr(), 1, None, dx.data_ptr(),
                                                   LN_WIDTH, None, dg2.data_ptr(), db2.data_ptr(), None, LN_ROWS, LN_WIDTH, 1e-5, handle),
                           "ln_bwd")
            s.synchronize()
            assert ops.reduce_stats() == (before + lapses, mreq), (nbytes, ops.reduce_stats())
            assert _relmax(dg2, ref["dgamma"].double()) < GATE
        for name, got in (("dx", dx), ("dgamma", dg), ("dbeta", db)):
            r = _relmax(got, ref[name].double())
            assert r < GATE, (name, r)
    finally:
        s.synchronize()
        _lib.check(lib.uniir_reduce_scratch(None, 0, handle), "reduce_scratch")
        ops.reset_reduce_stats()


def test_ops_grows_the_scratch_after_a_lapse(monkeypatch):
    """the same call three times through uniir_amd.ops on a fresh stream whose first buffer is 4 KiB: the first call lapses, the
    second finds the request in the counter, grows the buffer (one warning) and is reproducible, the third equals the second"""
    from uniir_amd import _lib, ops
    x, gamma, dy, ref = _ln_case()
    monkeypatch.setattr(ops, "RED_SCRATCH_BYTES", 4096)
    s = torch.cuda.Stream()
    key = (s.device.index, s.cuda_stream)
    assert key not in ops._RED_SCRATCH
    torch.cuda.synchronize()
    ops.reset_reduce_stats()
    res, falls = [], []
    try:
        with warnings.catch_warnings(record=True) as caught, torch.cuda.stream(s):
            warnings.simplefilter("always")
            for _ in range(3):
                dg, db = torch.zeros(LN_WIDTH, device=DEV), torch.zeros(LN_WIDTH, device=DEV)
                dx = ops.layernorm_bwd(x, gamma, dy, dg, db)
                s.synchronize()
                res.append(torch.cat([dg, db, dx.flatten()]))
                falls.append(ops.reduce_stats()[0])
        grown = [w for w in caught if "scratch" in str(w.message)]
        assert len(grown) == 1, [str(w.message) for w in caught]
        need = ops.reduce_stats()[1]
        assert str(1 << (need - 1).bit_length()) in str(grown[0].message)          # the warning names the new size
        assert ops._RED_SCRATCH[key].numel() == 1 << (need - 1).bit_length() >= need
        assert falls[0] >= 1 and falls[1] == falls[0] and falls[2] == falls[0], falls
        assert torch.equal(res[1], res[2])
        assert _relmax(res[1][:LN_WIDTH], ref["dgamma"].double()) < GATE and _relmax(res[0][:LN_WIDTH], ref["dgamma"].double()) < GATE
    finally:
        s.synchronize()
        _lib.load().uniir_reduce_scratch(None, 0, C.c_void_p(s.cuda_stream))
        ops._RED_SCRATCH.pop(key, None)
        ops.reset_reduce_stats()
