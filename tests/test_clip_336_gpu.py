"""The CLIP vision tower at 577 tokens (ViT-L/14@336px geometry: 336 pixels, 14-pixel patches, 24 x 24 + 1 tokens) on the streaming
attention kernels (csrc/attention_long.hip), against the CPU oracle (oracle/clip_oracle.py, fp32).  A tiny config with the real token
geometry: 2 layers, width 128 (2 heads), patch K = 588 padded to 640.  The gates are those of tests/test_clip_model_gpu.py and
tests/test_fp32_parity_gpu.py: the same arithmetic, longer rows."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))

NAME = "tiny-336-test"


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    return ((a - b).norm() / (b.norm() + 1e-20)).item()


def _cfg():
    from oracle import clip_oracle as O
    return O.tiny_config(image_resolution=336, vision_patch_size=14, vision_width=128, vision_layers=2, transformer_width=128,
                         transformer_heads=2, transformer_layers=2)


def _build(cfg, seed=0):
    from oracle import clip_oracle as O
    from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
    from uniir_amd import clip_model
    clip_model.CLIP_CONFIGS[NAME] = cfg
    sd = O.init_state_dict(cfg, seed=seed)
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    model = CLIPScoreFusion(NAME, device="cuda", config=config)
    model.clip_model.load_state_dict(sd, strict=True)
    return model, O.OracleCLIP(cfg, sd), O


def _batch(O, cfg, pairs=4, seed=11):
    batch = O.synthetic_batch(cfg, pairs, seed=seed)
    batch["image_mask_batched"][1] = 0          # item 1 text-only, item 2 image-only (clip_sf.py:61-62)
    batch["txt_mask_batched"][2] = 0
    return batch, {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _train_step(model, dbatch):
    """one training forward + backward from a clean gradient: embeddings, loss, the flat fp32 gradient"""
    clip = model.clip_model
    model.train()
    clip._ensure_flat()
    clip.zero_grad()
    emb = model.encode_multimodal_input(dbatch["txt_batched"], dbatch["image_batched"], dbatch["txt_mask_batched"],
                                        dbatch["image_mask_batched"]).detach().clone()
    out = model(dbatch)
    out["loss"].backward()
    torch.cuda.synchronize()
    return emb, float(out["loss"].detach()), clip._flat["g32"].clone()


def test_forward_backward_matches_oracle_at_577_tokens():
    cfg = _cfg()
    assert (cfg["image_resolution"] // cfg["vision_patch_size"]) ** 2 + 1 == 577
    model, oracle, O = _build(cfg)
    batch, dbatch = _batch(O, cfg)
    emb_o = O.encode_multimodal_input(oracle.sd(), cfg, batch["txt_batched"], batch["image_batched"],
                                      batch["txt_mask_batched"], batch["image_mask_batched"])
    out_o = O.inbatch_contrastive_loss(emb_o, batch["index_mapping"], oracle.logit_scale.exp())
    out_o["loss"].backward()
    model.train()
    model.clip_model._ensure_flat()
    model.clip_model.zero_grad()
    emb_d = model.encode_multimodal_input(dbatch["txt_batched"], dbatch["image_batched"], dbatch["txt_mask_batched"],
                                          dbatch["image_mask_batched"])
    print("OBS 336 emb rel", rel(emb_d, emb_o))
    assert rel(emb_d, emb_o) < 1.2e-2, rel(emb_d, emb_o)
    out_d = model(dbatch)
    print("OBS 336 loss diff", abs(out_d["loss"].item() - out_o["loss"].item()))
    assert abs(out_d["loss"].item() - out_o["loss"].item()) < 5e-3 * max(1.0, abs(out_o["loss"].item()))
    out_d["loss"].backward()
    errs = {}
    for n, p in model.clip_model.named_parameters():
        go = getattr(oracle, n.replace(".", "__")).grad
        if go is None:
            continue
        errs[n] = rel(p.grad, go)
    print("OBS 336 worst grad rel errs:", sorted(errs.items(), key=lambda kv: -kv[1])[:3])
    big = {n: e for n, e in errs.items() if e > 4e-2}
    assert not big, big
    gd = torch.cat([p.grad.flatten().cpu() for n, p in model.clip_model.named_parameters() if n in errs])
    go = torch.cat([getattr(oracle, n.replace(".", "__")).grad.flatten() for n, _ in model.clip_model.named_parameters() if n in errs])
    cos = torch.nn.functional.cosine_similarity(gd, go, dim=0).item()
    print("OBS 336 cos", cos)
    assert cos > 0.9995, cos


def test_recompute_blocks_equals_the_stored_step_at_577_tokens():
    cfg = _cfg()
    res = []
    for recompute in (False, True):
        model, _, O = _build(cfg, seed=5)
        model.clip_model.recompute_blocks = recompute
        model.clip_model.stash_act = True           # the stored run the recomputing one is bitwise equal to (act(f) kept)
        _, dbatch = _batch(O, cfg, seed=7)
        res.append(_train_step(model, dbatch))
    (e0, l0, g0), (e1, l1, g1) = res
    assert float(g0.abs().max()) > 0
    assert torch.equal(e0, e1)
    assert l0 == l1, (l0, l1)
    assert torch.equal(g0, g1), float((g0 - g1).abs().max())


def test_fp16_and_fp32_embeddings_against_the_oracle():
    """precision = "fp16" runs attn_long_fwd_kernel<true> (the only way to it): image embeddings within 1.5e-3, relative and per item,
    of the fp32 oracle (the gate of the ViT-L/14 fp16 test); precision = "fp32" within 2e-5 * max(1, |emb|max)"""
    cfg = _cfg()
    model, oracle, O = _build(cfg, seed=3)
    batch, dbatch = _batch(O, cfg, pairs=2)
    with torch.no_grad():
        emb_o = O.encode_image(oracle.sd(), batch["image_batched"], cfg)
    model.eval()
    clip = model.clip_model
    with torch.no_grad():
        clip.precision = "fp16"
        emb_h = clip.encode_image(dbatch["image_batched"]).float().cpu()
        clip.precision = "fp32"
        emb_f = clip.encode_image(dbatch["image_batched"]).float().cpu()
        clip.precision = "bf16"
    for r in range(emb_o.shape[0]):
        e = ((emb_h[r] - emb_o[r]).norm() / emb_o[r].norm()).item()
        print("OBS 336 fp16 item", r, e)
        assert e < 1.5e-3, (r, e)
    err = (emb_f - emb_o).abs().max().item()
    print("OBS 336 fp32 max abs", err)
    assert err < 2e-5 * max(1.0, float(emb_o.abs().max())), err


def test_pool_last_block_setting_changes_nothing_at_577_tokens():
    """above 512 tokens the vision tower runs its full last block whatever pool_last_block says (the text tower keeps its pooled
    block): embeddings and loss bitwise equal, and stash_log says so once"""
    cfg = _cfg()
    res = {}
    for pooled in (True, False):
        model, _, O = _build(cfg, seed=5)
        clip = model.clip_model
        clip.pool_last_block = pooled
        _, dbatch = _batch(O, cfg, seed=7)
        model.train()
        clip._ensure_flat()
        clip.zero_grad()
        temb, iemb = clip.encode_text(dbatch["txt_batched"]), clip.encode_image(dbatch["image_batched"])
        out = model(dbatch)
        out["loss"].backward()
        res[pooled] = (temb.detach().clone(), iemb.detach().clone(), float(out["loss"].detach()), list(clip.stash_log))
    p, f = res[True], res[False]
    assert torch.equal(p[0], f[0]) and torch.equal(p[1], f[1])
    assert p[2] == f[2], (p[2], f[2])
    lines = [s for s in p[3] if "full last block" in s]
    assert len(lines) == 1 and lines[0].startswith("image tower"), p[3]
    assert not [s for s in f[3] if "full last block" in s]


def test_two_identical_training_steps_give_the_same_bits_at_577_tokens():
    cfg = _cfg()
    grads = []
    for run in range(2):
        model, _, O = _build(cfg, seed=5)
        _, dbatch = _batch(O, cfg, seed=7)
        grads.append(_train_step(model, dbatch)[2])
    assert float(grads[0].abs().max()) > 0
    assert torch.equal(grads[0], grads[1])
