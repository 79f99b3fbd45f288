"""CLIP_FF with the token geometry of ViT-L/14@336px -- 577 image tokens (336 pixels, 14-pixel patches) + 77 text tokens = 654 fused
tokens, the T5 stack on the streaming relative-bias attention (uniir_attention_rel_fwd_long / _rel_bwd_long, csrc/attention_long.hip)
-- against the CPU oracle (oracle/clipff_oracle.py, fp32).  A tiny model with the real geometry: towers of 2 layers, width 128
(2 heads), T5 d_model 128, 2 heads, d_ff 256, 2 layers; 2 pairs (4 items).  The gates are those tests/test_clipff_gpu.py applies to
the same quantities (relative L2 < 2e-2 forward, the loss within 3e-2, deep_ok on the gradients);
tests/test_clipff_336_ref.py shows on the CPU that the oracle in bf16 meets them at this geometry with a factor two to spare.
Further: two identical train-mode steps give every parameter gradient bit for bit without a counted lapse, the step with block
recomputation equals the stored one, and the full-size model constructs."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))

from test_clipff_gpu import deep_ok, rel  # noqa: E402

NAME = "tiny-ff-336"
T5_CFG = dict(d_model=128, num_heads=2, d_ff=256, num_layers=2, d_kv=64)
PAIRS = 2
TOKENS = 77 + 577
T5_GRADS = ("block.0.layer.0.SelfAttention.q.weight", "block.0.layer.0.SelfAttention.o.weight", "block.1.layer.1.DenseReluDense.wi.weight",
            "block.1.layer.1.DenseReluDense.wo.weight", "block.0.layer.0.SelfAttention.relative_attention_bias.weight",
            "final_layer_norm.weight")
CLIP_GRADS = ("visual.proj", "visual.conv1.weight", "token_embedding.weight", "ln_final.weight",
              "visual.transformer.resblocks.0.attn.in_proj_weight")
DROP_P = 0.1
# The module draws every T5 matrix at fan_in^-0.5, so q and k have unit-variance elements and the un-scaled logits q.k a standard
# deviation of 8: softmaxes over 654 keys that are close to one-hot.  On such rows the oracle ITSELF in bf16 (tests/test_clipff_336_ref.py:
# autocast on the CPU, none of this project's kernels) is 10 % .. 17 % away from its own fp32 gradients (cosine 0.990): inside the gates
# below, but with less than the factor two a kernel should have.  transformers' T5 initialisation draws q at (d_model d_kv)^-0.5 --
# d_kv^-0.5 = 1 / 8 of the module's -- which gives logits of unit variance, where the bucketed bias (unit variance too) matters as much
# as q.k.  The tests therefore scale the q projections by Q_GAIN; the gates stay what they are.
Q_GAIN = T5_CFG["d_kv"] ** -0.5


def tiny_cfg():
    from oracle import clip_oracle as O
    return O.tiny_config(image_resolution=336, vision_patch_size=14, vision_width=128, vision_layers=2, transformer_width=128,
                         transformer_heads=2, embed_dim=128)


def build(device, dropout_rate=0.0, seed=5, q_gain=Q_GAIN):
    """the tiny model on `device` (the constructor needs no GPU; q_gain: see Q_GAIN), the oracle's state dict of the towers"""
    from oracle import clip_oracle as O
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from uniir_amd import clip_model
    cfg = tiny_cfg()
    clip_model.CLIP_CONFIGS[NAME] = cfg
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    m = CLIPFeatureFusion(NAME, device=device, config=config,
                          t5_config=dict(d_model=T5_CFG["d_model"], num_heads=T5_CFG["num_heads"], d_ff=T5_CFG["d_ff"],
                                         num_layers=T5_CFG["num_layers"], dropout_rate=dropout_rate))
    sd = O.init_state_dict(cfg, seed=seed)
    sd.pop("text_projection")
    m.clip_model.load_state_dict(sd, strict=True)
    with torch.no_grad():
        for n, p in m.t5_layers.named_parameters():
            if n.endswith("SelfAttention.q.weight"):
                p.mul_(q_gain)
    return m, sd, cfg


def t5_state(m):
    return {n: p.detach().cpu().clone() for n, p in m.t5_layers.named_parameters()}


def batch_of(cfg):
    from oracle import clip_oracle as O
    return O.synthetic_batch(cfg, PAIRS, seed=23)


def oracle_step(sd, t5sd, cfg, batch, bf16=False):
    """the oracle's embedding, loss and gradients of both stacks (CPU; bf16: every product under autocast)"""
    from oracle import clip_oracle as O
    from oracle import clipff_oracle as FF
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    t5o = {k: v.clone().requires_grad_(True) for k, v in t5sd.items()}
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
        emb = FF.encode_multimodal_input(sdo, t5o, cfg, T5_CFG, batch["txt_batched"], batch["image_batched"])
    out = O.inbatch_contrastive_loss(emb.float(), batch["index_mapping"], sdo["logit_scale"].exp())      # fp32, as the loss kernels are
    out["loss"].backward()
    grads = {n: t5o[n].grad for n in T5_GRADS}
    grads.update({n: sdo[n].grad for n in CLIP_GRADS})
    return emb.detach().float(), out, grads


def fusion_inputs():
    """token features of the 4 items as the towers would hand them to the stack, and the weights of the pooled output's gradient"""
    g = torch.Generator().manual_seed(41)
    M, D = 2 * PAIRS, T5_CFG["d_model"]
    return torch.randn(M, 77, D, generator=g), torch.randn(M, 577, D, generator=g), torch.randn(M, D, generator=g)


def oracle_dropout_step(t5sd, txt, img, w, masks, bf16=False):
    """the T5 stack with the six dropout sites as given masks: pooled output, gradient of the tokens, weight gradients"""
    from oracle import clipff_oracle as FF
    sdg = {k: v.clone().requires_grad_(True) for k, v in t5sd.items()}
    xo = torch.cat([txt, img], dim=1).clone().requires_grad_(True)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
        ref = FF.t5_stack(sdg, xo, T5_CFG, masks=masks).float().mean(dim=1)
    (ref * w).sum().backward()
    return ref.detach(), xo.grad, {n: sdg[n].grad for n in T5_GRADS}


def test_embedding_and_one_training_step_against_the_oracle():
    from uniir_amd.trainer import NativeAdamW
    m, sd, cfg = build("cuda")
    batch = batch_of(cfg)
    dbatch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    emb_o, out_o, g_o = oracle_step(sd, t5_state(m), cfg, batch)
    opt = NativeAdamW(m.clip_model, lr=1e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, allreduce=False,
                      extra=[m.t5_optimizer_group(lr=1e-3)])
    m.eval()
    with torch.no_grad():
        emb_d = m.encode_multimodal_input(dbatch["txt_batched"], dbatch["image_batched"])
    assert emb_d.shape == (2 * PAIRS, 128)
    print(f"\nOBS clipff-336 eval embedding rel {rel(emb_d, emb_o):.4g}")
    assert rel(emb_d, emb_o) < 2e-2, rel(emb_d, emb_o)
    m.train()
    opt.zero_grad()
    out_d = m(dbatch)
    out_d["loss"].backward()
    print(f"OBS clipff-336 loss {out_d['loss'].item():.6f} oracle {out_o['loss'].item():.6f}")
    assert abs(out_d["loss"].item() - out_o["loss"].item()) < 3e-2 * max(1.0, abs(out_o["loss"].item()))
    for name in T5_GRADS:
        deep_ok(m.t5_layers.get_parameter(name).grad, g_o[name], name)
    for name in CLIP_GRADS:
        deep_ok(m.clip_model.get_parameter(name).grad, g_o[name], name)
    w0 = m.t5_layers.get_parameter("block.0.layer.0.SelfAttention.q.weight").detach().clone()
    opt.step()
    assert (m.t5_layers.get_parameter("block.0.layer.0.SelfAttention.q.weight") - w0).abs().max().item() > 1e-4
    with torch.no_grad():
        dbatch["did_list"] = list(range(2 * PAIRS))
        emb, ids = m(dbatch, encode_mbeir_batch=True)
    assert emb.shape == (2 * PAIRS, 128) and torch.isfinite(emb).all()


def test_train_mode_dropout_step_matches_the_masked_oracle():
    """the six T5 dropout sites at 654 tokens with the exported counter-based masks fed to the oracle's hooks (the attention
    probabilities' among them: the DROP instantiations of the streaming kernels): pooled output, token gradient, weight gradients"""
    import numpy as np
    from uniir_amd import clipff_model as FM
    from uniir_amd import ops
    m, _, _ = build("cuda", dropout_rate=DROP_P)
    st = m._ensure_t5()
    m.zero_grad()
    txt, img, w = fusion_inputs()
    M, D = txt.shape[0], txt.shape[2]
    x = torch.cat([txt, img], dim=1).view(M * TOKENS, D).contiguous().cuda()
    torch.manual_seed(11)
    pooled, stash = FM.t5_forward(st, "", x.clone(), M, TOKENS, m.t5_heads, m.t5_layers_n, True, drop=ops.DropSeeds(), p=DROP_P)
    dx = FM.t5_backward(st, "", w.cuda(), stash, m.t5_heads, m.t5_layers_n).view(M, TOKENS, D)
    torch.manual_seed(11)
    seeds = ops.DropSeeds()

    def masks(kind, shape):
        buf = torch.empty(int(np.prod(shape)), device="cuda")
        ops.call("uniir_dropout_mask", buf, buf.numel(), DROP_P, seeds.next())
        return buf.view(*shape).cpu()

    ref, dxo, g_o = oracle_dropout_step(t5_state(m), txt, img, w, masks)
    plain, _, _ = oracle_dropout_step(t5_state(m), txt, img, w, None)
    print(f"\nOBS clipff-336 dropout pooled rel {rel(pooled, ref):.4g} (against the oracle without masks {rel(pooled, plain):.4g})")
    assert rel(pooled, ref) < 2e-2, rel(pooled, ref)
    assert rel(pooled, plain) > 5e-2
    deep_ok(dx, dxo, "dx")
    for name in T5_GRADS:
        deep_ok(st.grad_view(name), g_o[name], name)


def test_two_identical_train_steps_are_bitwise_equal_for_every_parameter():
    """train mode with dropout 0.1, the same seed before each step: after one warm-up step (it may grow the scratch) two steps give
    the same loss and the same gradient of every parameter of both stacks, and no reduction fell back to atomics"""
    from uniir_amd import ops
    m, _, cfg = build("cuda", dropout_rate=DROP_P)
    batch = batch_of(cfg)
    dbatch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    m.train()
    m.clip_model._ensure_flat()
    m._ensure_t5()

    def step():
        torch.manual_seed(7)
        m.zero_grad()
        out = m(dbatch)
        out["loss"].backward()
        torch.cuda.synchronize()
        grads = {"clip." + n: p.grad.detach().clone() for n, p in m.clip_model.named_parameters() if p.grad is not None}
        grads.update({"t5." + n: p.grad.detach().clone() for n, p in m.t5_layers.named_parameters() if p.grad is not None})
        return out["loss"].detach().clone(), grads

    step()
    ops.reset_reduce_stats()
    loss_a, a = step()
    loss_b, b = step()
    assert ops.reduce_stats()[0] == 0, ops.reduce_stats()
    assert torch.equal(loss_a, loss_b)
    assert set(a) == set(b) and len(a) > 50
    relb = [n for n in a if n.endswith("SelfAttention.relative_attention_bias.weight")]
    assert len(relb) == 1 and float(a[relb[0]].abs().max()) > 0
    for n, g in a.items():
        assert torch.equal(b[n], g), (n, float((b[n] - g).abs().max()), float(g.abs().max()))


def test_the_step_with_recompute_blocks_equals_the_stored_step():
    """CLIP.recompute_blocks (UNIIR_RECOMPUTE_BLOCKS) at 577 / 654 tokens: the towers' blocks rebuilt in the backward, eval-mode
    dropout off: the loss and every parameter gradient of both stacks are the stored step's bit for bit"""
    m, _, cfg = build("cuda")
    batch = batch_of(cfg)
    dbatch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    m.train()
    m.clip_model._ensure_flat()
    m._ensure_t5()
    res = []
    for recompute in (False, True, False):          # (the first step may grow the scratch: the last two are compared)
        m.clip_model.recompute_blocks = recompute
        m.zero_grad()
        out = m(dbatch)
        out["loss"].backward()
        torch.cuda.synchronize()
        grads = {"clip." + n: p.grad.detach().clone() for n, p in m.clip_model.named_parameters() if p.grad is not None}
        grads.update({"t5." + n: p.grad.detach().clone() for n, p in m.t5_layers.named_parameters() if p.grad is not None})
        res.append((out["loss"].detach().clone(), grads))
    m.clip_model.recompute_blocks = False
    assert any("block recomputation ON" in line for line in m.clip_model.stash_log)
    (la, a), (lb, b) = res[1], res[2]
    assert torch.equal(la, lb) and set(a) == set(b)
    for n, g in a.items():
        assert torch.equal(b[n], g), (n, float((b[n] - g).abs().max()), float(g.abs().max()))


def test_the_full_size_model_constructs():
    """CLIPFeatureFusion("ViT-L/14@336px"): the 336-pixel towers, a T5 stack of d_model 768, a 336-pixel preprocess; no forward"""
    from PIL import Image
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    m = CLIPFeatureFusion("ViT-L/14@336px", device="cuda")
    assert m.clip_model.cfg["image_resolution"] == 336
    assert tuple(m.t5_layers.get_parameter("block.0.layer.0.SelfAttention.q.weight").shape) == (768, 768)
    assert m.t5_layers.get_parameter("block.0.layer.0.SelfAttention.q.weight").is_cuda
    assert tuple(m.get_img_preprocess_fn()(Image.new("RGB", (500, 400))).shape) == (3, 336, 336)
