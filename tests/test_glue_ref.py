"""tests/glue_ref.py and tests/glue_cases.py tested on the CPU.

  * the references agree with independent torch formulations (F.unfold, F.embedding + autograd in fp64, torch.cat + broadcast add,
    .to(bfloat16 / float16), index_add_, plain loops);
  * an fp32 restatement of every bounded case, summed in another order than the kernels', stays at half of its bound or below;
  * planted defects are all caught: a dropped last row, a doubled row, an id clamped to the wrong end, truncation in place of
    round-to-nearest-even, a chunk shifted by 8, the mask indexed by the packed row in place of the logical row;
  * every case of the tables maps to the path it names through the restated host arithmetic, every path has a case, every grid-stride
    case strides with a ragged tail, and the integer data stays below 2^24.
No case is skipped or filtered."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import glue_cases as T
import glue_ref as G

BF16, F16 = torch.bfloat16, torch.float16


def _ratio(got, ref, bound, what):
    G.check(got, ref, bound, what)
    r = G.worst_ratio(got, ref, bound)
    assert r <= 0.5, f"{what}: a correct fp32 restatement at {r:.3f} of its bound -- the bound is too tight or its derivation wrong"
    return r


def _differs(got, want):
    with pytest.raises(AssertionError):
        G.assert_bits(got, want, "planted defect")


def _trunc_bf16(x):
    return (x.view(torch.int32) >> 16).to(torch.int16).view(BF16)


# ================================================================================================================ exact references
@pytest.mark.parametrize("name,n,res,P,kpad", T.PATCHIFY, ids=[c[0] for c in T.PATCHIFY])
def test_patchify_is_unfold(name, n, res, P, kpad):
    img = torch.randn(n, 3, res, res, generator=torch.Generator().manual_seed(res))
    ref = G.patchify(img, P, kpad)
    g = res // P
    unf = F.unfold(img, P, stride=P).transpose(1, 2).reshape(n * g * g, 3 * P * P)
    G.assert_bits(ref[:, :3 * P * P].contiguous(), unf.to(BF16), name)
    assert ref.shape == (n * g * g, kpad) and bool((ref[:, 3 * P * P:].view(torch.int16) == 0).all())
    # the header's index formula on a few elements
    for row, k in ((0, 0), (n * g * g - 1, 3 * P * P - 1), (g * g // 2, P * P + P + 1)):
        im, gy, gx = row // (g * g), (row // g) % g, row % g
        c, py, px = k // (P * P), (k % (P * P)) // P, k % P
        assert float(ref[row, k]) == float(img[im, c, gy * P + py, gx * P + px].to(BF16))
    _differs(_trunc_bf16(unf), ref[:, :3 * P * P].contiguous())                       # truncation in place of RNE
    shifted = torch.roll(ref, 8, 1)
    _differs(shifted, ref)                                                           # a chunk shifted by 8


@pytest.mark.parametrize("n,T_,w", T.ASSEMBLE)
def test_vit_assemble_is_cat_plus_pos(n, T_, w):
    g = torch.Generator().manual_seed(w)
    po, cls, pos = torch.randn(n * (T_ - 1), w, generator=g), torch.randn(w, generator=g), torch.randn(T_, w, generator=g)
    for src in (po.to(BF16), po):
        want = (torch.cat([cls.expand(n, 1, w), src.float().view(n, T_ - 1, w)], 1) + pos[None]).view(n * T_, w)
        G.assert_bits(G.vit_assemble(src, cls, pos, n, T_), want, "vit_assemble")
    dx, dc0, dp0 = torch.randn(n * T_, w, generator=g), torch.randn(w, generator=g), torch.randn(T_, w, generator=g)
    b = G.vit_assemble_bwd(dx, n, T_, dc0, dp0)
    xr = dx.double().view(n, T_, w)
    assert torch.allclose(b["dpos"].double(), dp0.double() + xr.sum(0), rtol=0, atol=float(G.gamma(n + 1) * (xr.abs().sum(0) + 1).max() * 2))
    assert torch.allclose(b["dclass"].double(), dc0.double() + xr[:, 0].sum(0), rtol=0, atol=1e-5 * n)
    G.assert_bits(b["dpatch"], dx.view(n, T_, w)[:, 1:].reshape(-1, w).to(BF16), "dpatch")
    if n > 1:                                                                        # a dropped last item, a doubled item
        _differs(G.vit_assemble_bwd(dx[:-T_], n - 1, T_, dc0, dp0)["dpos"], b["dpos"])
        _differs(G.vit_assemble_bwd(torch.cat([dx, dx[-T_:]]), n + 1, T_, dc0, dp0)["dpos"], b["dpos"])


def test_chain_sum_is_the_sequential_sum():
    t = torch.randn(9, 5, generator=torch.Generator().manual_seed(1))
    s = np.zeros(5, np.float32)
    for i in range(9):
        s = (s + t[i].numpy()).astype(np.float32)
    G.assert_bits(G.chain_sum(t), torch.from_numpy(s), "chain")
    live = torch.tensor([1, 0, 1, 1, 0, 0, 1, 1, 1], dtype=torch.bool)
    G.assert_bits(G.chain_sum(t, live[:, None].expand(9, 5)), G.chain_sum(t[live]), "chain with skipped items")


@pytest.mark.parametrize("n,ctx,w,vocab,oob", T.TEXT)
def test_text_embed_is_embedding(n, ctx, w, vocab, oob):
    g = torch.Generator().manual_seed(vocab)
    text = torch.randint(-3 if oob else 0, vocab + (3 if oob else 0), (n, ctx), generator=g).to(torch.int32)
    text[0, 0] = -2 if oob else 0
    text[-1, -1] = vocab + 1 if oob else vocab - 1
    tok, pos = torch.randn(vocab, w, generator=g), torch.randn(ctx, w, generator=g)
    x, eot = G.text_embed(text, tok, pos, vocab)
    want = F.embedding(text.long().clamp(0, vocab - 1), tok) + pos
    G.assert_bits(x, want.view(n * ctx, w), "text_embed")
    for i in range(n):                                                              # first arg-max, ties included
        row = text[i].tolist()
        assert int(eot[i]) == row.index(max(row))
    if oob:                                                                          # an id clamped to the wrong end
        wrong = F.embedding(torch.where(text.long() < 0, vocab - 1, text.long().clamp(0, vocab - 1)), tok) + pos
        if vocab > 1:
            _differs(wrong.view(n * ctx, w), x)
    lens = torch.randint(1, ctx + 1, (n,), generator=g).to(torch.int32)
    lens[0] = ctx
    xp, last = G.text_embed_packed(text, tok, pos, vocab, lens)
    rows = [want[i, :int(lens[i])] for i in range(n)]
    G.assert_bits(xp, torch.cat(rows), "packed")
    assert last.tolist() == [int(lens[:i + 1].sum()) - 1 for i in range(n)]


def test_eot_ties_take_the_first():
    text = torch.tensor([[5, 9, 2, 9], [7, 7, 7, 7], [0, 1, 2, 3], [-4, -9, -4, -5]], dtype=torch.int32)
    _, eot = G.text_embed(text, torch.zeros(10, 4), torch.zeros(4, 4), 10)
    assert eot.tolist() == [1, 0, 3, 0]


def test_text_gradients_are_autograd():
    c = T.TOK[3]
    for packed in (False, True):
        lens = T.tok_lens(c) if packed else None
        text = T.tok_text(c, lens=lens)
        rows = int(lens.sum()) if packed else c.rows
        dx, dtok0, dpos0 = T.tok_data(c, rows, False)
        tok = torch.zeros(c.vocab, c.w, dtype=torch.float64, requires_grad=True)
        pos = torch.zeros(c.ctx, c.w, dtype=torch.float64, requires_grad=True)
        x = F.embedding(G.clamp_ids(text, c.vocab), tok) + pos
        x = x[G.live_mask(lens, c.ctx)] if packed else x.view(rows, c.w)
        x.backward(dx.double())
        ref, bound = G.dtok(text, dx, c.vocab, dtok0, True, lens)
        assert float((ref - (dtok0.double() + tok.grad)).abs().max()) < 1e-12
        dpos = G.text_dpos(dx, c.n, c.ctx, dpos0, lens)
        assert float((dpos.double() - (dpos0.double() + pos.grad)).abs().max()) < 1e-5
        assert float(bound.max()) < 1e-4


@pytest.mark.parametrize("n,seq,w,kind", T.GATHER)
def test_gather_scatter_are_index_ops(n, seq, w, kind):
    total = n * seq if seq else 3 * n
    g = torch.Generator().manual_seed(n)
    x, dout = torch.randn(total, w, generator=g), torch.randn(n, w, generator=g)
    idx = T.gather_idx(n, seq, kind, total)
    r = [i * seq + (int(idx[i]) if idx is not None else 0) for i in range(n)]
    assert len(set(r)) == n and max(r) < total
    G.assert_bits(G.gather_rows(x, idx, n, seq), torch.stack([x[j] for j in r]), "gather")
    want = x.clone().index_add_(0, torch.tensor(r), dout)
    G.assert_bits(G.scatter_rows(dout, idx, x, seq), want, "scatter")


def test_cast_references():
    x = torch.randn(7, 5)
    for dt in (BF16, F16):
        p = G.cast_pad_rows(x, 8, dt)
        assert p.shape == (7, 8) and bool((p[:, 5:].view(torch.int16) == 0).all())
        G.assert_bits(p[:, :5].contiguous(), x.to(dt), "cast_pad_rows")
    b = G.cast_inputs(BF16).to(BF16)
    assert torch.equal(G.bf16_to_f32(b).view(torch.int32), b.float().view(torch.int32))


def test_cast_inputs_hold_the_edges():
    xb, xh = G.cast_inputs(BF16), G.cast_inputs(F16)
    assert xb.numel() == 4 * 65536 + 6 and xh.numel() >= 4 * 63488
    fmax_b = torch.tensor([0x7F7F8000], dtype=torch.int32).view(torch.float32)      # the tie above bf16's largest finite value
    assert bool((xb.view(torch.int32) == 0x7F7F8000).any()) and bool(torch.isinf(fmax_b.to(BF16)).all())
    for v in (65504.0, 65520.0, -65520.0, 2.0 ** -24, 2.0 ** -25, 2.0 ** -14, 0.0):
        assert bool((xh == v).any()), v
    assert bool(torch.isinf(torch.tensor(65520.0).to(F16))) and float(torch.tensor(2.0 ** -25).to(F16)) == 0.0
    below = float(np.nextafter(np.float32(2.0 ** -25), np.float32(0)))
    assert bool((xh == below).any()) and float(torch.tensor(below).to(F16)) == 0.0
    for x in (xb, xh):
        assert bool(torch.isnan(x).any()) and bool(torch.isinf(x).any()) and bool(((x != 0) & (x.abs() < G.TINY32)).any())
        z = x.view(torch.int32)
        assert bool((z == 0).any()) and bool((z == -0x80000000).any())
    # ties: both neighbours of the midpoint are 16-bit values and the cast picks the even one
    mid = xh[63488:2 * 63488]
    assert torch.equal(mid.to(F16).view(torch.int16) & 1, torch.zeros(mid.numel(), dtype=torch.int16)) or bool(torch.isinf(mid.to(F16)).any())


@pytest.mark.parametrize("dt", [BF16, F16], ids=["bf16", "f16"])
def test_cast_verdict(dt):
    x = G.cast_inputs(dt)
    good = x.to(dt)
    bad, nsub, ieee, zero = G.cast_verdict(x, good, dt)
    assert not bool(bad.any()) and ieee == nsub and zero == 0 and nsub > 0
    # flushed fp32 subnormals are accepted, with the sign; anything else flushed is not
    sub = (x != 0) & (x.abs() < G.TINY32)
    flushed = torch.where(sub, torch.copysign(torch.zeros_like(x), x).to(dt), good)
    bad, _, _, zero = G.cast_verdict(x, flushed, dt)
    assert not bool(bad.any()) and (zero > 0 or dt == F16)
    wrong_sign = torch.where(sub, torch.copysign(torch.zeros_like(x), -x).to(dt), good)
    assert bool(G.cast_verdict(x, wrong_sign, dt)[0].any())
    # truncation in place of round-to-nearest-even
    if dt == BF16:
        assert int(G.cast_verdict(x, _trunc_bf16(x), dt)[0].sum()) > 60000
    else:
        toward0 = torch.where(good.float().abs() > x.abs(), (good.view(torch.int16) - 1).view(F16), good)
        assert int(G.cast_verdict(x, toward0, dt)[0].sum()) > 30000
    # a NaN turned into a number, a payload changed
    nan = torch.isnan(x)
    assert bool(G.cast_verdict(x, torch.where(nan, torch.zeros_like(good), good), dt)[0].any())
    other = torch.where(nan, torch.full_like(good, float("nan")), good)
    assert not bool(G.cast_verdict(x, other, dt)[0].any())


# ======================================================================================================================= dropout
def _fmix_py(i, seed):
    h = (i * 0x9E3779B1 ^ seed) & 0xFFFFFFFF
    h ^= h >> 16
    h = h * 0x85EBCA6B & 0xFFFFFFFF
    h ^= h >> 13
    h = h * 0xC2B2AE35 & 0xFFFFFFFF
    return h ^ (h >> 16)


def test_drop_mask_restatement():
    assert _fmix_py(0, 0) == 0 and int(G.drop_hash(np.array([0]), 0)[0]) == 0
    idx = np.array([0, 1, 2, 1000, 2 ** 31, 2 ** 32 - 1])
    for seed in (0, 77, 0xFFFFFFFF):
        assert [int(h) for h in G.drop_hash(idx, seed)] == [_fmix_py(int(i), seed) for i in idx]
    assert G.drop_threshold(0.0) == 0 and G.drop_threshold(1e-10) == 0 and G.drop_threshold(0.5) == 2 ** 31
    assert G.drop_threshold(T.P_TOP) == 4294967040 and float(G.keep_scale(T.P_TOP)) == 2.0 ** 24
    assert float(G.keep_scale(0.1)) == float(np.float32(1.0) / np.float32(np.float32(1.0) - np.float32(0.1)))
    m = G.drop_mask(400, 260, 0.1, 5)
    kept = float((m != 0).mean())
    assert abs(kept - 0.9) < 0.01 and set(np.unique(m)) == {np.float32(0.0), G.keep_scale(0.1)}
    assert bool((G.drop_mask(37, 8, 1e-10, 5) == 1.0).all()) and bool((G.drop_mask(37, 8, 0.0, 5, always_hash=True) == 1.0).all())
    assert float((G.drop_mask(400, 260, T.P_TOP, 5) != 0).mean()) < 1e-3
    # the packed rows draw the logical rows' elements
    rm = np.array([5, 0, 399, 17])
    assert np.array_equal(G.drop_mask(4, 260, 0.5, 9, rm), G.drop_mask(400, 260, 0.5, 9)[rm])
    assert not np.array_equal(G.drop_mask(4, 260, 0.5, 9, rm), G.drop_mask(4, 260, 0.5, 9))      # indexed by the packed row: caught


@pytest.mark.parametrize("c", T.DROP, ids=[c.name for c in T.DROP])
def test_dropout_forms(c):
    x, resid, rowscale, row_map = T.drop_data(c)
    f = G.drop_factor(G.drop_mask(c.rows, c.cols, c.p, c.seed), rowscale, c.div or 1)
    r = resid.numpy() if c.resid else None
    forms = G.dropout_forms(x.numpy(), f, r)
    prod = x * torch.from_numpy(f)
    two = (prod + resid if c.resid else prod).numpy()
    ok, only_two, only_fused, both = G.dropout_accepts(two, forms)
    assert ok.all() and only_fused == 0 and only_two + both == two.size
    if c.resid and c.p in (0.1, 0.5) and c.rows * c.cols >= 256:
        assert only_two > 0, "the two forms never differ on this data: the split would say nothing"
    prod = x.double() * torch.from_numpy(f).double()
    fused = (prod + resid.double() if c.resid else prod).float().numpy()
    assert G.dropout_accepts(fused, forms)[0].all()
    assert G.dropout_accepts(G.to_bf16_np(fused), forms, bf16=True)[0].all()
    if c.p not in (0.0, 1e-10):
        off = G.drop_factor(G.drop_mask(c.rows, c.cols, c.p, c.seed + 1), rowscale, c.div or 1)
        if not np.array_equal(off, f):
            assert not G.dropout_accepts(G.dropout_forms(x.numpy(), off, r)[0], forms)[0].all()
    if c.div:
        assert c.rows % c.div != 0
    want = (x.to(BF16).float() * torch.from_numpy(f)).to(BF16)
    G.assert_bits(G.dropout_bf16(x.to(BF16), f), want, "dropout_bf16")
    assert len(set(row_map.tolist())) == c.rows and int(row_map.max()) >= c.rows          # a strict subset, not the identity


# ========================================================================================================================= sums
@pytest.mark.parametrize("c", T.COLSUM, ids=[c.name for c in T.COLSUM])
def test_colsum_case(c):
    plan = T.colsum_plan(c.rows, c.cols, c.out_off % 4 == 0, c.scratch)
    assert plan["form"] == c.path, (c.name, plan)
    assert plan["fallbacks"] == (1 if c.path == "atomic" else 0) and (plan["bytes"] == plan["gy"] * c.cols * 4 or c.path == "one")
    assert c.cols % 8 == 0 and c.pad % 8 == 0
    depth = G.colsum_depth(plan["rpb"], plan["gy"])
    x, out0 = T.colsum_data(c, True)
    ref, bound = G.colsum(x, out0, depth)
    assert float(bound.max()) == 0.0 and float(x.float().abs().sum(0).max() + 9) < 2.0 ** 24
    exact = out0 + x.float().sum(0)
    assert torch.equal(exact.double(), ref)
    if c.rows > 1:
        lost = out0 + x[:-1].float().sum(0)                                          # a dropped last row, a doubled row
        assert bool(G.violations(lost, ref, bound).any())
        assert bool(G.violations(exact + x[0].float(), ref, bound).all() | (x[0] == 0).any())
    x, out0 = T.colsum_data(c, False)
    ref, bound = G.colsum(x, out0, depth)
    h = c.rows // 2
    got = out0 + (x[h:].float().sum(0) + x[:h].float().sum(0))
    _ratio(got, ref, bound, c.name)
    if c.rows > 1:
        assert bool(G.violations(out0 + x[:-1].float().sum(0), ref, bound).any())


def _tok_setup(c, packed, integer):
    lens = T.tok_lens(c) if packed else None
    text = T.tok_text(c, lens=lens)
    rows = int(lens.sum()) if packed else c.rows
    cnt = G.token_counts(text, c.vocab, lens)
    plan = T.tok_plan(c, c.rows, int(cnt.max()))
    dx, dtok0, dpos0 = T.tok_data(c, rows, integer)
    return lens, text, cnt, plan, dx, dtok0, dpos0


@pytest.mark.parametrize("packed", [False, True], ids=["dense", "packed"])
@pytest.mark.parametrize("c", T.TOK, ids=[c.name for c in T.TOK])
def test_tok_case(c, packed):
    lens, text, cnt, plan, dx, dtok0, dpos0 = _tok_setup(c, packed, True)
    assert plan["form"] == c.path, (c.name, plan)
    assert plan["fallbacks"] == (1 if c.path == "atomic" else 0)
    assert [int(cnt[i + 1]) for i in range(len(c.buckets))] == list(c.buckets)
    assert int(cnt[0]) > 0 and int(cnt[c.vocab - 1]) > 0
    if c.oob:
        assert int(text.min()) < 0 and int(text.max()) >= c.vocab
    if c.straddle:
        long_id = len(c.buckets)
        assert int(text.flatten()[4095]) == long_id and int(text.flatten()[4096]) == long_id and c.buckets[-1] > T.TOKD_SORT
    if packed:
        assert int(lens.min()) == 1 and int(lens.max()) == c.ctx and int(lens.sum()) < c.rows
    fixed = c.path != "atomic"
    ref, bound = G.dtok(text, dx, c.vocab, dtok0, fixed, lens, plan["nslices"])
    assert float(bound.max()) == 0.0, "the integer data leaves the exact range"
    ids = G.clamp_ids(text, c.vocab)
    ids = ids[G.live_mask(lens, c.ctx)] if packed else ids.flatten()
    exact = dtok0.clone().index_add_(0, ids, dx)
    assert torch.equal(exact.double(), ref)
    # a dropped last row, a doubled row, an id clamped to the wrong end
    assert bool(G.violations(dtok0.clone().index_add_(0, ids[:-1], dx[:-1]), ref, bound).any()) or not bool(dx[-1].any())
    assert bool(G.violations(exact.clone().index_add_(0, ids[:1], dx[:1]), ref, bound).any()) or not bool(dx[0].any())
    if c.oob and c.vocab > 1:
        raw = text[G.live_mask(lens, c.ctx)] if packed else text.flatten()
        wrong = torch.where(raw.long() < 0, c.vocab - 1, raw.long().clamp(0, c.vocab - 1))
        assert bool(G.violations(dtok0.clone().index_add_(0, wrong, dx), ref, bound).any())
    lens, text, cnt, plan, dx, dtok0, dpos0 = _tok_setup(c, packed, False)
    ref, bound = G.dtok(text, dx, c.vocab, dtok0, fixed, lens, plan["nslices"])
    order = torch.argsort(ids, stable=True).flip(0)                                  # another order: descending rows per id
    got = dtok0.clone().index_add_(0, ids[order], dx[order])
    _ratio(got, ref, bound, c.name)
    # a row lost from a short bucket (an arrival-order sum of 4097 rows has a bound wider than one row: the integer run is the
    # check that loses none there)
    keep = torch.ones(ids.numel(), dtype=torch.bool)
    keep[int(cnt[ids].argmin())] = False
    assert bool(G.violations(dtok0.clone().index_add_(0, ids[keep], dx[keep]), ref, bound).any())


def test_every_path_has_a_case():
    assert {c.path for c in T.TOK} == T.TOK_PATHS and {c.path for c in T.COLSUM} == T.COLSUM_PATHS
    assert {c.w for c in T.TOK} >= {4, 252, 256, 260} and {c.vocab for c in T.TOK} >= {1, 1023, 1024, 1025, 30524, 49408, 65536, 65537}
    assert set(T.BUCKETS) <= {b for c in T.TOK for b in c.buckets}
    assert {c.rows for c in T.COLSUM} >= {1, 3, 4, 5, 63, 64, 65, 1000} and {c.cols for c in T.COLSUM} >= {8, 504, 512, 520, 776}
    assert any(c.pad for c in T.COLSUM) and {c.scratch for c in T.COLSUM} == {"on", "off", "short"}
    assert {c.scratch for c in T.TOK} == {"on", "off", "short"} and any(c.dx_off for c in T.TOK) and any(c.dtok_off for c in T.TOK)
    assert any(c.rows <= 4096 and c.buckets for c in T.TOK)
    assert {(P, res // P) for _, _, res, P, _ in T.PATCHIFY} >= {(16, 1), (16, 2), (14, 16), (32, 1)}
    assert {k for *_, k in T.PATCHIFY} >= {768, 592, 640}
    for _, _, res, P, kpad in T.PATCHIFY:
        assert res % P == 0 and kpad % 8 == 0 and kpad >= 3 * P * P
    assert {T_ for _, T_, _ in T.ASSEMBLE} >= {2, 197} and {w for *_, w in T.ASSEMBLE} >= {4, 260, 768} and any(n == 1 for n, *_ in T.ASSEMBLE)
    assert {k for *_, k in T.GATHER} == {"none", "item", "abs"}
    assert {c.p for c in T.DROP} >= set(T.DROP_P) and {c.outs for c in T.DROP} == {"f32", "bf16", "both"}
    assert any(not c.resid for c in T.DROP) and any(c.div and c.rows % c.div for c in T.DROP) and any(c.pad and c.div for c in T.DROP)
    assert {n for n, _ in T.INV_NORMS} == {1, 63, 64, 65, 257} and {d for _, d in T.INV_NORMS} == {8, 64, 72, 768}


STRIDED = [("patchify", (T.PATCHIFY_BIG[1], T.PATCHIFY_BIG[2] // T.PATCHIFY_BIG[3], T.PATCHIFY_BIG[4])),
           ("vit_assemble", T.ASSEMBLE_BIG), ("vit_assemble_f32", T.ASSEMBLE_F32_BIG), ("text_embed", T.TEXT_BIG[:3]),
           ("text_embed_packed", T.TEXT_BIG[:3]), ("gather_rows", (T.GATHER_BIG[0], T.GATHER_BIG[2])),
           ("scatter_rows", (T.GATHER_BIG[0], T.GATHER_BIG[2])), ("act_fwd", (T.ACT_BIG,)), ("cast_f32_to_bf16", (T.CAST_BIG,)),
           ("cast_f32_to_f16", (T.CAST_BIG,)), ("cast_bf16_to_f32", (T.BF16_F32_BIG,)), ("cast_pad_rows", (T.PAD_ROWS_BIG[0], T.PAD_ROWS_BIG[2])),
           ("unpad_add", T.UNPAD_BIG[:2]), ("tanh_fwd", (T.TANH_BIG,)), ("tanh_bwd", (T.TANH_BIG,)),
           ("dropout_f32", (T.DROP_BIG.rows, T.DROP_BIG.cols)), ("dropout_f32_rows", (T.DROP_BIG.rows, T.DROP_BIG.cols)),
           ("dropout_bf16", (T.DROP_BIG.rows, T.DROP_BIG.cols)), ("dropout_bf16_rows", (T.DROP_BIG.rows, T.DROP_BIG.cols)),
           ("dropout_mask", (T.DROP_MASK_BIG,))]


@pytest.mark.parametrize("kernel,dims", STRIDED, ids=[k for k, _ in STRIDED])
def test_strided_cases_stride(kernel, dims):
    grid, work, trips = T.trips(kernel, *dims)
    assert grid == T.CAPS[kernel][0] and trips == 2 and 0 < work - grid * 256 < grid * 256, (kernel, grid, work)
    assert work % 256 != 0 or kernel in ("cast_f32_to_bf16", "cast_f32_to_f16")       # a ragged last block (the casts: a live tail)
    assert set(T.CAPS) == {k for k, _ in STRIDED}
    assert T.grid_for(1) == 1 and T.grid_for(0) == 1 and T.grid_for(257) == 2 and T.grid_for(10 ** 9, 256, 16384) == 16384


def test_small_cases_do_not_stride():
    for _, n, res, P, kpad in T.PATCHIFY:
        assert T.trips("patchify", n, res // P, kpad)[2] == 1
    assert T.CAST_BIG % 4 == 3


# =================================================================================================================== activations
def _act32(x, act, defect=None):
    x = x.numpy().astype(np.float32)
    one, half = np.float32(1.0), np.float32(0.5)
    with np.errstate(all="ignore"):
        if act == G.QUICK_GELU:
            t = np.float32(1.702 if defect != "coef" else 1.72) * x
            y = x * (one / (one + np.exp(-t)))
        elif act == G.ERF_GELU:
            ax = np.abs(x)
            t = one / (ax * np.float32(0.23164189) + one)
            E = np.exp(np.float32(-0.5) * x * x)
            poly = t * np.float32(1.061405429) + np.float32(-1.453152027)
            for cf in (1.421413741, -0.284496736, 0.254829592 if defect != "coef" else 0.26):
                poly = t * poly + np.float32(cf)
            q = (half * t) * (poly * E)
            y = x * np.where(x >= 0, one - q, q)
        else:
            y = np.maximum(x, np.float32(0.0)) if defect != "coef" else np.maximum(x, np.float32(-1e-3))
    return torch.from_numpy(y.astype(np.float32)).to(BF16)


@pytest.mark.parametrize("act", [G.QUICK_GELU, G.ERF_GELU, G.RELU], ids=["quickgelu", "erfgelu", "relu"])
def test_act_bounds_on_every_bf16_value(act):
    x = T.all_bf16().float()
    fin = torch.isfinite(x)
    ref, bound = G.act_fwd(x[fin], act)
    got = _act32(x[fin], act)
    r = _ratio(got, ref, bound, f"act {act}")
    print(f"\nOBS act {act} fp32 restatement worst ratio {r:.3f}")
    assert bool(G.violations(_act32(x[fin], act, "coef"), ref, bound).any())
    sp = G.act_special(x[~fin], act)
    assert bool(torch.isnan(sp[torch.isnan(x[~fin])]).all())
    pinf, ninf = torch.tensor([float("inf")]), torch.tensor([float("-inf")])
    assert float(G.act_special(pinf, act)) == float("inf")
    assert bool(torch.isnan(G.act_special(ninf, act))) if act != G.RELU else float(G.act_special(ninf, act)) == 0.0
    if act == G.RELU:
        assert float(bound.max()) == 0.0


def test_tanh_bounds():
    x, dy = T.tanh_data(4099)
    ref, bound = G.tanh_fwd(x)
    y = torch.tanh(x)
    _ratio(y, ref, bound, "tanh_fwd")
    assert bool(G.violations(torch.tanh(x * 1.0001), ref, bound).any())
    ref, bound = G.tanh_bwd(y, dy)
    _ratio(dy * (1.0 - y * y), ref, bound, "tanh_bwd")
    _ratio(torch.addcmul(dy, dy * y, y, value=-1.0), ref, bound, "tanh_bwd, other association")
    assert bool(G.violations(dy * (1.0 - y), ref, bound).any())


# ==================================================================================================================== inv norms
@pytest.mark.parametrize("n,dim", T.INV_NORMS)
def test_inv_norms_chain(n, dim):
    x = T.inv_norm_data(n, dim)
    got = G.inv_norms(x)
    v = x.float().numpy()
    s = np.zeros(n, np.float32)
    for j in range(dim):
        s = (s + (v[:, j] * v[:, j]).astype(np.float32)).astype(np.float32)
    with np.errstate(divide="ignore"):
        want = np.where(s > 0, (1.0 / np.sqrt(s).astype(np.float64)).astype(np.float32), np.float32(0.0))
    G.assert_bits(got, torch.from_numpy(want), "inv_norms")
    assert float(got[n // 2]) == 0.0 and (n == 1 or float(got.max()) > 0)
