"""The fp32 embedding forward of CLIP_FF (CLIPFeatureFusion.precision = "fp32": clip_model's fp32 tower blocks without pooling, the T5
stack on uniir_sgemm / uniir_attn_f32_rel_fwd / uniir_rmsnorm_fwd's fp32 output) against oracle/clipff_oracle.py, with the measured
gate of tests/test_blip_embed_fp32_gpu.py: E32 = the largest difference between the oracle on fp32 and on .double() tensors, the device
within 16 * E32 of the fp64 oracle (and of the reference golden where one exists: G12's pooled output, G13's embedding), the "fp16"
output of the seeded model outside the gate by a factor of 4 at least.

The oracles spell some fp32 casts `.float()` (upstream's LayerNorm subclass, T5's softmax); on fp64 tensors those would round the
reference back to fp32, so the fp64 evaluation runs with Tensor.float keeping fp64 tensors as they are (_double_stays_double)."""
import contextlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))
G = os.path.join(ROOT, "tests", "golden")

from test_blip_embed_fp32_gpu import APART, FACTOR, _cast, _maxdiff  # noqa: E402
from test_clipff_gpu import _model as small_model  # noqa: E402


@contextlib.contextmanager
def _double_stays_double():
    real = torch.Tensor.float
    torch.Tensor.float = lambda self, *a, **k: self if self.dtype == torch.float64 else real(self, *a, **k)
    try:
        yield
    finally:
        torch.Tensor.float = real


def _gate(what, got, oracle, golden=None):
    """test_blip_embed_fp32_gpu._gate with the fp64 evaluation under _double_stays_double"""
    with torch.no_grad():
        o32 = oracle(torch.float32)
        with _double_stays_double():
            o64 = oracle(torch.float64)
    assert o32.dtype == torch.float32 and o64.dtype == torch.float64 and got.dtype == torch.float32 and tuple(got.shape) == tuple(o64.shape)
    e32, err = _maxdiff(o32, o64), _maxdiff(got, o64)
    line = f"\nOBS {what}: E32 {e32:.3e} device fp32 error {err:.3e} = {err / e32:.2f} E32 (gate {FACTOR:.0f})"
    if golden is not None:
        eg = _maxdiff(got, golden)
        line += f"; against the reference golden {eg:.3e} = {eg / e32:.2f} E32"
    print(line)
    assert e32 > 0 and bool(torch.isfinite(got).all())
    assert err <= FACTOR * e32, (what, err, e32)
    if golden is not None:
        assert eg <= FACTOR * e32, (what, "golden", eg, e32)
    return e32, o64


def _stack_on_the_golden(z, x):
    """the fp32 T5 stack of a model that carries the golden's T5 weights on token features x [M, T, D] -> pooled [M, D], the weights"""
    from oracle import clip_oracle as O
    from uniir_amd import clipff_model as FM
    t5_cfg = json.loads(str(z["cfg"]))
    cfg = O.tiny_config(embed_dim=t5_cfg["d_model"], transformer_width=t5_cfg["d_model"], transformer_heads=2)
    m, _ = small_model(cfg, t5_cfg)
    sd = {k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    m.t5_layers.load_state_dict(sd, strict=True)
    st = m._ensure_t5()
    M, T, D = x.shape
    with torch.no_grad():
        pooled = FM.t5_forward_f32(st, "", x.cuda().view(M * T, D).contiguous(), M, T, m.t5_heads, m.t5_layers_n)
    return pooled, sd, t5_cfg


def test_g12_t5_stack_alone():
    from oracle import clipff_oracle as FF
    z = np.load(os.path.join(G, "g12_t5stack.npz"))
    x = torch.from_numpy(z["x"])
    pooled, sd, t5_cfg = _stack_on_the_golden(z, x)
    _gate("g12 T5 stack pooled", pooled, lambda dt: FF.t5_stack(_cast(sd, dt), x.to(dt), t5_cfg).mean(dim=1), golden=z["pooled"])


def test_g13_fusion_of_the_reference_token_features():
    from oracle import clipff_oracle as FF
    z = np.load(os.path.join(G, "g13_clipff.npz"))
    txt, img = torch.from_numpy(z["txt_feat"]), torch.from_numpy(z["img_feat"])
    pooled, sd, t5_cfg = _stack_on_the_golden(z, torch.cat([txt, img], dim=1))
    _gate("g13 CLIP_FF fusion embedding", pooled, lambda dt: FF.fuse_tokens(_cast(sd, dt), txt.to(dt), img.to(dt), t5_cfg),
          golden=z["emb"])


NAME = "tiny-ff-336-w64"
T5_CFG = dict(d_model=64, num_heads=2, d_ff=128, num_layers=2, d_kv=64)


def _tiny_336(seed=5):
    """a seeded CLIP_FF with the token geometry of ViT-L/14@336px: 77 + 577 = 654 fused tokens, width 64, one layer per tower, two T5
    layers (q projections at transformers' scale, tests/test_clipff_336_gpu.py Q_GAIN) -> model (eval), the towers' state dict, cfg, batch"""
    from oracle import clip_oracle as O
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from uniir_amd import clip_model
    cfg = O.tiny_config(image_resolution=336, vision_patch_size=14, vision_width=64, vision_layers=1, transformer_width=64,
                        transformer_heads=1, transformer_layers=1, embed_dim=64)
    clip_model.CLIP_CONFIGS[NAME] = cfg
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    m = CLIPFeatureFusion(NAME, device="cuda", config=config,
                          t5_config=dict(d_model=T5_CFG["d_model"], num_heads=T5_CFG["num_heads"], d_ff=T5_CFG["d_ff"],
                                         num_layers=T5_CFG["num_layers"], dropout_rate=0.0))
    sd = O.init_state_dict(cfg, seed=seed)
    sd.pop("text_projection")
    m.clip_model.load_state_dict(sd, strict=True)
    with torch.no_grad():
        for n, p in m.t5_layers.named_parameters():
            if n.endswith("SelfAttention.q.weight"):
                p.mul_(T5_CFG["d_kv"] ** -0.5)
    m.embed_fp16 = False          # whatever the environment says: the tests set what they test
    m.embed_fp32 = True           # the module opted in: without that "fp32" is no precision it knows (the guards test)
    return m.eval(), sd, cfg, O.synthetic_batch(cfg, 1, seed=23)


def _encode(m, precision, txt, img, masks=(None, None)):
    was = m.precision
    m.precision = precision
    try:
        with torch.no_grad():
            return m.encode_multimodal_input(txt, img, *masks).clone()
    finally:
        m.precision = was


def test_654_fused_tokens_every_mask_combination_and_the_gate_tells_fp32_from_fp16():
    from oracle import clipff_oracle as FF
    m, sd, cfg, batch = _tiny_336()
    t5sd = {n: p.detach().cpu().clone() for n, p in m.t5_layers.named_parameters()}
    txt, img = batch["txt_batched"], batch["image_batched"]
    assert cfg["context_length"] + (cfg["image_resolution"] // cfg["vision_patch_size"]) ** 2 + 1 == 654
    got = _encode(m, "fp32", txt.cuda(), img.cuda())
    assert not got.requires_grad
    e32, o64 = _gate("654 tokens CLIP_FF", got,
                     lambda dt: FF.encode_multimodal_input(_cast(sd, dt), _cast(t5sd, dt), cfg, T5_CFG, txt, img.to(dt)))
    half = _encode(m, "fp16", txt.cuda(), img.cuda())
    eh = _maxdiff(half, o64)
    print(f"\nOBS 654 tokens CLIP_FF: fp16 error {eh:.3e} = {eh / e32:.1f} E32 (outside the gate by {eh / (FACTOR * e32):.1f}x, wanted {APART:.0f}x)")
    assert eh >= APART * FACTOR * e32, (eh, e32)
    # the masks are accepted and unused, like in the reference (clip_ff.py:161-192): every combination is the same forward
    n = txt.shape[0]
    ones, zeros = torch.ones(n, dtype=torch.int64).cuda(), torch.zeros(n, dtype=torch.int64).cuda()
    for masks in ((ones, ones), (ones, zeros), (zeros, ones)):
        assert torch.equal(_encode(m, "fp32", txt.cuda(), img.cuda(), masks), got)
    dbatch = {"txt_batched": txt.cuda(), "image_batched": img.cuda(), "txt_mask_batched": None, "image_mask_batched": None,
              "did_list": list(range(n))}
    m.precision = "fp32"
    with torch.no_grad():          # through the reference surface, too
        e1, ids1 = m.encode_mbeir_batch(dbatch)
        e2, _ = m(dbatch, encode_mbeir_batch=True)
    assert torch.equal(e1, got) and torch.equal(e2, got) and ids1 == dbatch["did_list"]


def test_guards_on_the_device_and_the_bf16_path_is_untouched():
    m, sd, cfg, batch = _tiny_336()
    txt, img = batch["txt_batched"].cuda(), batch["image_batched"].cuda()
    emb0 = _encode(m, "bf16", txt, img)
    m.precision, m.embed_fp32 = "fp32", False
    with pytest.raises(RuntimeError, match="unknown precision 'fp32'"), torch.no_grad():          # a module that has not opted in
        m.encode_multimodal_input(txt, img)
    m.embed_fp32 = True
    with pytest.raises(RuntimeError, match="no_grad"):          # grad enabled
        m.encode_multimodal_input(txt, img)
    m.train()
    with pytest.raises(RuntimeError, match="eval"), torch.no_grad():
        m.encode_multimodal_input(txt, img)
    m.eval()
    m.precision = "fp64"
    with pytest.raises(RuntimeError, match="unknown precision"), torch.no_grad():
        m.encode_multimodal_input(txt, img)
    m.precision = "bf16"
    f = _encode(m, "fp32", txt, img)
    assert m.clip_model._flat.h16_buf is None and m._t5.h16_buf is None          # fp32 reads the masters: no fp16 shadow is built
    assert not torch.equal(f, emb0) and torch.equal(_encode(m, "bf16", txt, img), emb0)
