"""The fp16 forward of the BLIP vision encoder (BLIPFeatureFusion._vit_tokens(precision="fp16"): blip_model.vit_forward with
dtype16 = torch.float16 over the online store's fp16 shadow) against oracle/blip_oracle.py in fp32, next to the bf16 forward on the
same inputs.

The bound on the ratio is the project's figure for "three more mantissa bits", 0.35 (tests/test_fp32_parity_gpu.py asserts it for the
CLIP towers): every 16-bit rounding on the way -- operands, activations, the returned tokens -- has a relative step of 2^-11 in fp16
and 2^-8 in bf16, a factor of 8, and nothing else differs between the two forwards (fp32 residual stream, statistics and
accumulation in both); 0.35 leaves the fp32 parts of the error, which do not shrink, a share of almost three in eight.
The bf16 bound 2e-2 is that of tests/test_blip_gpu.py."""
import json
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
RATIO = 0.35
MED_TINY = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=1, vocab_size=64,
                max_position_embeddings=32)


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def tiny_model(med_cfg, vit_cfg, seed=0):
    from uniir_amd.blip_model import BLIPFeatureFusion
    return BLIPFeatureFusion(med_config=med_cfg, vit_config=vit_cfg, embed_dim=med_cfg["hidden_size"], queue_size=16, momentum=0.9,
                             config=types.SimpleNamespace(tokenizer_max_length=20), seed=seed)


def _oracle_tokens(model, images):
    from oracle import blip_oracle as bo
    sd = {n[len("visual_encoder."):]: p.detach().cpu().float() for n, p in model.named_parameters() if n.startswith("visual_encoder.")}
    with torch.no_grad():
        return bo.vit_forward(sd, images.cpu().float(), model.vit_cfg)


def _both_against_the_oracle(model, images, what):
    want = _oracle_tokens(model, images)
    b = model._vit_tokens(images, "bf16")
    h = model._vit_tokens(images, "fp16")
    assert b.dtype == torch.bfloat16 and h.dtype == torch.float16 and b.shape == h.shape == want.shape
    rb, rh = rel(b.float(), want), rel(h.float(), want)
    print(f"OBS {what} rel_bf16 {rb:.3e} rel_fp16 {rh:.3e} ratio {rh / rb:.3f}")
    assert rb < 2e-2, (what, rb)
    assert rh < RATIO * rb, (what, rh, rb)
    return b, h


def test_g7_tokens_fp16_beats_bf16_against_the_oracle():
    z = np.load(os.path.join(G, "g7_vit.npz"))
    model = tiny_model(MED_TINY, json.loads(str(z["cfg"]))).cuda().eval()
    sd = {"visual_encoder." + k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd::")}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    x = torch.from_numpy(z["x"]).cuda()
    _, h = _both_against_the_oracle(model, x, "g7")
    y = torch.from_numpy(z["y"])          # the reference's own output
    assert rel(h.float().view(y.shape), y) < 2e-2


def test_577_tokens_run_the_streaming_fp16_attention(monkeypatch):
    """384 pixels: 577 tokens, above what a workgroup holds in LDS -- every block's attention is the streaming kernel behind
    uniir_attention_fwd_f16, counted at the library call"""
    from uniir_amd import _lib
    vit_cfg = dict(img_size=384, patch_size=16, embed_dim=128, depth=2, num_heads=2, drop_path_rate=0.0)
    model = tiny_model(MED_TINY, vit_cfg, seed=5).cuda().eval()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 384, 384, generator=g).cuda()
    lib = _lib.load()
    real, seen = lib.uniir_attention_fwd_f16, []

    def counted(qkv, out, lse, row_off, batch, seq, heads, causal, stream):
        seen.append((row_off, batch, seq, heads, causal))
        return real(qkv, out, lse, row_off, batch, seq, heads, causal, stream)

    monkeypatch.setattr(lib, "uniir_attention_fwd_f16", counted)
    _both_against_the_oracle(model, x, "577 tokens")
    assert seen == [(None, 2, 577, 2, 0)] * 2          # one call per block, dense rows, no mask


def test_real_widths_1024_wide_16_heads_197_tokens():
    """ViT-L/16's widths (1024-wide rows, 16 heads, 4096-wide MLP, 197 tokens) at two blocks and two images"""
    vit_cfg = dict(img_size=224, patch_size=16, embed_dim=1024, depth=2, num_heads=16, drop_path_rate=0.1)
    model = tiny_model(MED_TINY, vit_cfg, seed=3).cuda().eval()
    g = torch.Generator().manual_seed(7)
    _both_against_the_oracle(model, torch.randn(2, 3, 224, 224, generator=g).cuda(), "ViT-L widths")


def _g8():
    z = np.load(os.path.join(G, "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    b = len(z["s0_pdid"])
    batch = {"txt_batched": types.SimpleNamespace(input_ids=torch.from_numpy(z["s0_ids"]).cuda(),
                                                  attention_mask=torch.from_numpy(z["s0_mask"]).cuda()),
             "image_batched": torch.from_numpy(z["s0_img"]).cuda(), "p_did_list": torch.from_numpy(z["s0_pdid"]),
             "index_mapping": {"query": [[2 * i] for i in range(b)], "pos_cand": [[2 * i + 1] for i in range(b)]}}
    return med_cfg, vit_cfg, batch


def test_the_fp16_copies_follow_the_fused_adamw_and_in_place_edits():
    """one bf16 training step with the project's AdamW (which writes the master weights and the bf16 shadow itself), then fp16
    tokens: those of a fresh model that loaded the stepped state_dict, bit for bit -- and again after an in-place edit of a weight"""
    from uniir_amd.trainer import NativeAdamW
    med_cfg, vit_cfg, batch = _g8()
    model = tiny_model(med_cfg, vit_cfg).cuda()
    x = batch["image_batched"]
    model.eval()
    before = model._vit_tokens(x, "fp16").clone()          # the fp16 copies exist BEFORE the weights move
    model.train()
    opt = NativeAdamW(model, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, allreduce=False)
    opt.zero_grad()
    model(batch, alpha=0.4)["loss"].backward()
    opt.step()
    model.eval()
    got = model._vit_tokens(x, "fp16")
    assert not torch.equal(got, before)

    def fresh():
        m = tiny_model(med_cfg, vit_cfg, seed=9).cuda().eval()
        m.load_state_dict(model.state_dict())
        return m._vit_tokens(x, "fp16")

    assert torch.equal(got, fresh())
    with torch.no_grad():
        model.get_parameter("visual_encoder.blocks.0.mlp.fc1.weight")[3, :7] += 0.5
        model.get_parameter("visual_encoder.patch_embed.proj.weight")[1, 0, 2, :5] -= 0.25
    got2 = model._vit_tokens(x, "fp16")
    assert not torch.equal(got2, got) and torch.equal(got2, fresh())
    # the momentum update (EMA kernel) leaves the online copies valid and the result unchanged
    model._momentum_update()
    assert torch.equal(model._vit_tokens(x, "fp16"), got2)


def test_guards_and_the_bf16_path_is_untouched():
    from uniir_amd import blip_model as bm
    med_cfg, vit_cfg, batch = _g8()
    model = tiny_model(med_cfg, vit_cfg).cuda().eval()
    x = batch["image_batched"]
    with torch.no_grad():
        emb0 = model.encode_multimodal_input(batch["txt_batched"], x).clone()
    tok0 = model._vit_tokens(x).clone()
    assert model._online.h16_buf is None and model._online.half_bytes() == 0          # bf16 users allocate nothing
    with pytest.raises(RuntimeError, match="unknown precision"):
        model._vit_tokens(x, "fp32")
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model._vit_tokens(x, "fp16")
    model.eval()
    h = model._vit_tokens(x, "fp16")
    assert h.dtype == torch.float16 and model._online.h16_buf is not None and model._mom.h16_buf is None
    assert h.requires_grad is False
    st = model._online
    with pytest.raises(RuntimeError, match="save=True"):          # no fp16 stash: nothing to run a backward from
        bm.vit_forward(st, "visual_encoder.", model.vit_cfg, model.image_size, x, True, dtype16=torch.float16)
    # (an fp16 forward can no longer be handed the bf16 patch weight: vit_forward takes the one of its dtype16 from the store)
    assert st.padded16h("visual_encoder.patch_embed.proj.weight").dtype == torch.float16 and st.half_bytes() > 2 * st.total
    # after fp16 was used: the bf16 tokens and the model's embeddings are what they were before, bit for bit
    assert torch.equal(model._vit_tokens(x, "bf16"), tok0)
    with torch.no_grad():
        assert torch.equal(model.encode_multimodal_input(batch["txt_batched"], x), emb0)
    tok, T, _ = bm.vit_forward(st, "visual_encoder.", model.vit_cfg, model.image_size, x, False)
    assert torch.equal(tok.view(tok0.shape), tok0)
