"""Block recomputation in the per-op towers (uniir_amd/resblocks.py tower_fwd's recompute_from): the BLIP ViT under the reference's
vit_grad_ckpt / vit_ckpt_layer keys and CLIP_FF's two towers without pooling under CLIP.recompute_blocks.  A recomputed block keeps only
its fp32 input; tower_bwd rebuilds the rest with block_sublayers -- the forward's own function, arguments and deterministic kernels --
right before that block's backward.  So nothing may differ from the stored run: every comparison below is torch.equal / float equality
with the default reproducible reductions, except the one gradient the project documents as an arrival-order atomic sum (the T5
relative-position bias)."""
import os
import sys
import types
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))

VIT = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2)         # 17 tokens
MED = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=2, vocab_size=64,
           max_position_embeddings=32)


def tiny_model(med_cfg, vit_cfg, queue_size=16, momentum=0.9, cls=None, **kw):
    from uniir_amd.blip_model import BLIPFeatureFusion
    return (cls or BLIPFeatureFusion)(med_config=med_cfg, vit_config=vit_cfg, embed_dim=med_cfg["hidden_size"],
                                      queue_size=queue_size, momentum=momentum,
                                      config=types.SimpleNamespace(tokenizer_max_length=20), **kw)


def _first_difference(a, b):
    d = (a != b).flatten().nonzero()
    return None if d.numel() == 0 else (int(d[0]), int(d.shape[0]))


# ---- 1. ViT blocks, function level ----------------------------------------------------------------------------------------------
def _vit_run(model, x, dtok, k, seed=13):
    from uniir_amd import blip_model as bm
    from uniir_amd import ops
    st = model._online
    model.zero_grad()
    torch.manual_seed(seed)                                     # the DropPath draw (torch's CPU generator): the same rowscale
    drop = ops.DropSeeds() if model.training else None
    tok, T, stash = bm.vit_forward(st, "visual_encoder.", model.vit_cfg, model.image_size, x, True, drop=drop,
                                   recompute_from=k)
    kept = [len(e) for e in stash["saved"]]
    inputs_only = all(e[0].dtype == torch.float32 and e[0].shape == (x.shape[0] * T, model.vit_cfg["embed_dim"])
                      for e in stash["saved"])
    rowscale = stash["rowscale"]
    bm.vit_backward(st, "visual_encoder.", model.vit_cfg, dtok, stash)
    torch.cuda.synchronize()
    return tok.clone(), st.g32.clone(), kept, inputs_only, rowscale


@pytest.mark.parametrize("train", [False, True])
def test_vit_blocks_recomputed_equal_stored(train):
    """depth 4, 6 images of 17 tokens = 102 rows (no multiple of the 16-row attention tiles or of any GEMM tile); boundaries 4 (none),
    2 and 0 (all); eval mode and train mode with DropPath 0.5 (rowscale stored once, read again by the rebuild)"""
    depth, M = VIT["depth"], 6
    vit_cfg = dict(VIT, drop_path_rate=0.5) if train else dict(VIT)
    model = tiny_model(MED, vit_cfg, seed=3).cuda()
    model.train(train)
    model._sync()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, 3, 64, 64, generator=g).cuda()
    dtok = torch.randn(M * 17, 128, generator=g).cuda()
    tok0, g0, kept0, _, rs0 = _vit_run(model, x, dtok, depth)
    assert kept0 == [8] * depth
    assert (rs0 is not None) == train
    if train:
        assert float(rs0.min()) == 0.0 and float(rs0.max()) > 1.0            # some branch dropped, some kept and scaled
    blocks = [n for n, _ in model._online_params() if "visual_encoder.blocks." in n]
    assert len(blocks) == 12 * depth
    assert all(float(model._online.grad_view(n).abs().max()) > 0 for n in blocks)
    for k in (depth, 2, 0):
        tok, gk, kept, inputs_only, rs = _vit_run(model, x, dtok, k)
        assert kept == [8] * k + [1] * (depth - k), kept                    # a recomputed block's entry: its input and nothing else
        assert inputs_only
        if train:
            assert torch.equal(rs, rs0)
        assert torch.equal(tok, tok0), (k, float((tok.float() - tok0.float()).abs().max()))
        assert torch.equal(gk, g0), (k, _first_difference(gk, g0), float((gk - g0).abs().max()))


# ---- 2. memory -------------------------------------------------------------------------------------------------------------------
def test_vit_peak_memory_drops_by_the_rebuilt_sets():
    """width 512, 8 heads, 8 blocks, 384 images of 17 tokens = 6528 rows.  A stored block keeps its input plus one set
    (block_set_bytes); a recomputed one its input alone, and one shared set exists during the forward and one during the backward.
    Everything else the two runs allocate is the same, so the peak drops by (depth - 1) sets; 0.9 of it is required -- the slack of
    tests/test_recompute_gpu.py for the caching allocator's rounding.  One unmeasured forward + backward first, so that every lazily
    created buffer exists before the measured one."""
    from uniir_amd import blip_model as bm
    from uniir_amd.resblocks import block_set_bytes
    vit_cfg = dict(img_size=64, patch_size=16, embed_dim=512, depth=8, num_heads=8)
    med = dict(MED, hidden_size=512, num_attention_heads=8, intermediate_size=512, num_hidden_layers=1)
    model = tiny_model(med, vit_cfg, seed=4).cuda()
    model.eval()
    model._sync()
    st = model._online
    M, T, W = 384, 17, 512
    R = M * T
    assert R == 6528
    g = torch.Generator().manual_seed(6)
    x = torch.randn(M, 3, 64, 64, generator=g).cuda()
    dtok = torch.randn(R, W, generator=g).cuda()

    def step(k):
        tok, _, stash = bm.vit_forward(st, "visual_encoder.", model.vit_cfg, model.image_size, x, True,
                                       recompute_from=k)
        bm.vit_backward(st, "visual_encoder.", model.vit_cfg, dtok, stash)
        del tok, stash
        torch.cuda.synchronize()

    peaks = {}
    for k in (8, 0):
        model.zero_grad()
        step(k)
        model.zero_grad()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step(k)
        peaks[k] = torch.cuda.max_memory_allocated() - base
    want = (8 - 1) * block_set_bytes(R, W, 8)
    drop = peaks[8] - peaks[0]
    print(f"OBS per-op recompute peak: stored {peaks[8]} B, recomputed {peaks[0]} B, drop {drop} B, seven block sets {want} B")
    assert want > (512 << 20), want
    assert drop >= 0.9 * want, (drop, want)


# ---- 3. BLIP_FF / BLIP_SF, model level -------------------------------------------------------------------------------------------
def _blip_batch(pairs=4, L=20):
    g = torch.Generator().manual_seed(8)
    n = 2 * pairs
    ids = torch.randint(3, MED["vocab_size"], (n, L), generator=g)
    ids[:, 0] = 1
    valid = torch.tensor([L, 1, 7, 12, 20, 3, 9, 15])[:n]
    mask = (torch.arange(L).unsqueeze(0) < valid.unsqueeze(1)).long()
    return {"txt_batched": types.SimpleNamespace(input_ids=(ids * mask).cuda(), attention_mask=mask.cuda()),
            "image_batched": torch.randn(n, 3, 64, 64, generator=g).cuda(),
            "p_did_list": torch.arange(100, 100 + pairs),
            "index_mapping": {"query": [[2 * i] for i in range(pairs)], "pos_cand": [[2 * i + 1] for i in range(pairs)]}}


def _blip_step(score_fusion, ckpt):
    from uniir_amd.blip_model import BLIPFeatureFusion, BLIPScoreFusion
    med = dict(MED, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    vit = dict(VIT, drop_path_rate=0.1)
    model = tiny_model(med, vit, cls=BLIPScoreFusion if score_fusion else BLIPFeatureFusion, seed=9, vit_grad_ckpt=ckpt,
                       vit_ckpt_layer=2).cuda()
    assert model.vit_recompute_from == (2 if ckpt else 4)
    model.train()
    torch.manual_seed(31)
    model.zero_grad()
    out = model(_blip_batch(), alpha=0.3)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model._online_params() if n not in model._frozen}
    return dict(loss=float(out["loss"].detach()), grads=grads, g32=model._online.g32.clone(), mom=model._mom.p32.clone(),
                queues=(model.query_queue.clone(), model.cand_queue.clone(), model.idx_queue.clone(), model.new_ptr_queue.clone()))


@pytest.mark.parametrize("score_fusion", [False, True])
def test_blip_step_with_vit_grad_ckpt_equals_the_stored_step(score_fusion):
    """4 pairs, train mode (BERT dropout 0.1, DropPath 0.1), one model(batch, alpha) + backward: vit_grad_ckpt=True, vit_ckpt_layer=2
    (blocks 2 and 3 of 4 recomputed) against False.  First the stored step against itself: the precondition of the comparison."""
    s0, s1 = _blip_step(score_fusion, False), _blip_step(score_fusion, False)
    rc = _blip_step(score_fusion, True)
    for other, what in ((s1, "stored, repeated"), (rc, "recomputed")):
        assert other["loss"] == s0["loss"], (what, other["loss"], s0["loss"])
        assert set(other["grads"]) == set(s0["grads"])
        for n, g in s0["grads"].items():
            assert torch.equal(other["grads"][n], g), (what, n, float((other["grads"][n] - g).abs().max()), float(g.abs().max()))
        assert torch.equal(other["g32"], s0["g32"]), (what, _first_difference(other["g32"], s0["g32"]))
        assert torch.equal(other["mom"], s0["mom"]), what
        for a, b in zip(other["queues"], s0["queues"]):
            assert torch.equal(a, b), what
    vit_w = [n for n in s0["grads"] if "visual_encoder.blocks." in n and n.endswith("weight")]
    assert len(vit_w) == 6 * VIT["depth"] and all(float(s0["grads"][n].abs().max()) > 0 for n in vit_w)


# ---- 4. / 5. CLIP_FF -------------------------------------------------------------------------------------------------------------
T5 = dict(d_model=128, num_heads=2, d_ff=256, num_layers=2, d_kv=64)


def _clipff_cfg(**kw):
    from oracle import clip_oracle as O
    return O.tiny_config(vision_width=128, vision_layers=3, transformer_width=128, transformer_heads=2, transformer_layers=3, **kw)


def _clipff_model(cfg, seed=5):
    from oracle import clip_oracle as O
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from uniir_amd import clip_model
    clip_model.CLIP_CONFIGS["tiny-ff-recompute"] = cfg
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    m = CLIPFeatureFusion("tiny-ff-recompute", device="cuda", config=config,
                          t5_config=dict(d_model=T5["d_model"], num_heads=T5["num_heads"], d_ff=T5["d_ff"],
                                         num_layers=T5["num_layers"], dropout_rate=0.0))
    sd = O.init_state_dict(cfg, seed=seed)
    sd.pop("text_projection")
    m.clip_model.load_state_dict(sd, strict=True)
    return m


def test_clipff_towers_recomputed_equal_stored():
    """3 + 3 blocks of width 128, 6 items: vision_tokens_fwd / _bwd and text_tokens_fwd / _bwd with CLIP.recompute_blocks on and off on
    fixed dtok -- tokens and the whole flat gradient buffer bitwise; block_done sees L-1 .. 0 once per tower in both modes"""
    from oracle import clip_oracle as O
    from uniir_amd import clipff_model as FM
    cfg = _clipff_cfg()
    L = 3
    m = _clipff_model(cfg)
    clip = m.clip_model
    clip._sync_shadow()
    batch = O.synthetic_batch(cfg, 3, seed=23)
    text = batch["txt_batched"].to(torch.int32).cuda().contiguous()
    image = batch["image_batched"].cuda().contiguous()
    assert text.shape[0] == 6 and image.shape[0] == 6
    calls = []
    clip.block_done = lambda prefix: (lambda i: calls.append((prefix, i)))
    g = torch.Generator().manual_seed(2)
    dts = {}
    res = {}
    for recompute in (False, True):
        clip.recompute_blocks = recompute
        clip.zero_grad()
        calls.clear()
        ttok, Tt, tst = FM.text_tokens_fwd(clip, text, True)
        itok, Ti, ist = FM.vision_tokens_fwd(clip, image, True)
        if not dts:
            dts["t"] = torch.randn(ttok.shape, generator=g).cuda()
            dts["i"] = torch.randn(itok.shape, generator=g).cuda()
        kept = ([len(e) for e in tst["saved"]], [len(e) for e in ist["saved"]])
        assert kept == (([1] * L, [1] * L) if recompute else ([8] * L, [8] * L)), kept
        FM.text_tokens_bwd(clip, dts["t"], tst)
        FM.vision_tokens_bwd(clip, dts["i"], ist)
        torch.cuda.synchronize()
        assert calls == [("transformer", i) for i in reversed(range(L))] + [("visual.transformer", i) for i in reversed(range(L))], calls
        res[recompute] = (ttok.clone(), itok.clone(), clip._flat["g32"].clone())
    clip.recompute_blocks = False
    assert float(res[False][2].abs().max()) > 0
    assert torch.equal(res[True][0], res[False][0]) and torch.equal(res[True][1], res[False][1])
    assert torch.equal(res[True][2], res[False][2]), _first_difference(res[True][2], res[False][2])


def _clipff_step(cfg, dbatch, recompute):
    m = _clipff_model(cfg)
    clip = m.clip_model
    clip.recompute_blocks = recompute
    m.train()
    clip._ensure_flat()
    m._ensure_t5()
    m.zero_grad()
    emb = m.encode_multimodal_input(dbatch["txt_batched"], dbatch["image_batched"])
    assert emb.requires_grad
    out = m(dbatch)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {"clip." + n: p.grad.detach().clone() for n, p in clip.named_parameters() if p.grad is not None}
    grads.update({"t5." + n: p.grad.detach().clone() for n, p in m.t5_layers.named_parameters() if p.grad is not None})
    return dict(loss=out["loss"].detach().clone(), emb=emb.detach().clone(), grads=grads, log=list(clip.stash_log))


def test_clipff_step_with_recompute_blocks_equals_the_stored_step():
    """the whole CLIP_FF model, dropout 0, 4 pairs: loss, fused embeddings and every parameter gradient bitwise, except the T5
    relative-position bias (an arrival-order atomic scatter-add in the stored mode too, INTEGRATION.md "still order-dependent"), which is
    held to the project's 5e-2 relative gradient gate.  One "recomputation" log line per tower with the switch on, none with it off."""
    from oracle import clip_oracle as O
    cfg = _clipff_cfg(embed_dim=128)             # the fusion stack reads both towers' tokens at one width
    batch = O.synthetic_batch(cfg, 4, seed=23)
    dbatch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    st = _clipff_step(cfg, dbatch, False)
    rc = _clipff_step(cfg, dbatch, True)
    assert sum("recomputation" in s for s in rc["log"]) == 2, rc["log"]
    assert any(s.startswith("text tower") for s in rc["log"]) and any(s.startswith("image tower") for s in rc["log"])
    assert not any("recomputation" in s for s in st["log"]), st["log"]
    assert torch.equal(rc["loss"], st["loss"]), (rc["loss"], st["loss"])
    assert torch.equal(rc["emb"], st["emb"])
    assert set(rc["grads"]) == set(st["grads"]) and len(st["grads"]) > 80
    atomic = [n for n in st["grads"] if n.endswith("SelfAttention.relative_attention_bias.weight")]
    assert len(atomic) == 1
    for n, g in st["grads"].items():
        if n in atomic:
            r = float((rc["grads"][n] - g).norm() / g.norm().clamp_min(1e-20))
            assert r < 5e-2, (n, r)
        else:
            assert torch.equal(rc["grads"][n], g), (n, float((rc["grads"][n] - g).abs().max()), float(g.abs().max()))
    assert all(float(g.abs().max()) > 0 for n, g in st["grads"].items() if "resblocks" in n and "weight" in n)
