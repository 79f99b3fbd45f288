"""The fp32 embedding forward of BLIP_FF and BLIP_SF (BLIPFeatureFusion.precision = "fp32": blip_model.vit_forward_f32 /
bert_forward_f32 on the fp32 masters of the online store) against oracle/blip_oracle.py.

The gate is measured, not fixed: E32 is the largest difference between the oracle on fp32 tensors and the same functions on
.double() tensors (the oracles are plain functions of a state dict), and the device's fp32 output must be within 16 * E32 of the fp64
oracle.  Why 16: the device's GEMM sums K sequentially in 4-wide MFMA chains, up to 4 * width long, torch's CPU GEMM sums in blocks;
the device's expf / erff / tanhf differ from torch's by a few ulp.  The device's result is another valid fp32 evaluation, with an error
of the same order but not the same value; a logic error (a mask constant, an eps of 1e-6 for 1e-12) shows at 1e-3 or more.  Where a
reference golden exists for an output (G6: pooler_output and last_hidden_state; G7: the tokens) the device is held to 16 * E32 of it
as well.  The seeded 384-pixel model also shows that the gate tells the precisions apart: its "fp16" output is outside by a factor of
4 at least.  Every figure is printed (OBS lines; profiles/embed_fp32.txt keeps one run's)."""
import json
import os
import types

import numpy as np
import pytest
import torch

from test_blip_gpu import load_sub, tiny_model

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
FACTOR, APART = 16.0, 4.0
L = 20


def _cast(sd, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in sd.items()}


def _maxdiff(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _gate(what, got, oracle, golden=None):
    """oracle(dtype) -> the oracle's output on tensors of that dtype.  Prints and asserts; -> (E32, the fp64 oracle's output)"""
    with torch.no_grad():
        o32, o64 = oracle(torch.float32), oracle(torch.float64)
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


def _model(score_fusion, med_cfg, vit_cfg, embed_dim=None, seed=0):
    from uniir_amd import blip_model as bm
    cls = bm.BLIPScoreFusion if score_fusion else bm.BLIPFeatureFusion
    m = cls(med_config=med_cfg, vit_config=vit_cfg, embed_dim=embed_dim or med_cfg["hidden_size"], queue_size=16, momentum=0.9,
            config=types.SimpleNamespace(tokenizer_max_length=L), seed=seed)
    m.pool_last_layer = m.embed_fp16 = False          # whatever the environment says: the tests set what they test
    m.embed_fp32 = True                               # the module opted in: without that "fp32" is no precision it knows (the guards test)
    return m


def _encode(model, precision, txt, img, masks=(None, None)):
    was = model.precision
    model.precision = precision
    try:
        with torch.no_grad():
            return model.encode_multimodal_input(txt, img, *masks).clone()
    finally:
        model.precision = was


def test_g6_med_bert_multimodal_and_text_mode_with_the_padding_mask():
    from oracle import blip_oracle as bo
    from uniir_amd import blip_model as bm
    z = np.load(os.path.join(G, "g6_med.npz"))
    med_cfg = json.loads(str(z["cfg"]))
    vit_cfg = dict(img_size=32, patch_size=16, embed_dim=med_cfg["encoder_width"], depth=1, num_heads=2)
    model = tiny_model(med_cfg, vit_cfg).cuda().eval()
    sd = load_sub(model, z, "sd::", "text_encoder.")
    sd = {k[len("text_encoder."):]: v for k, v in sd.items()}
    model._sync()
    st, cfg = model._online, model.med_cfg
    ids, mask, img = torch.from_numpy(z["ids"]), torch.from_numpy(z["mask"]), torch.from_numpy(z["img"])
    assert int(mask.sum()) < mask.numel()          # the padding mask is on
    n, Ti, Ew = img.shape
    dids, key_len = ids.to(torch.int32).cuda(), mask.sum(1).to(torch.int32).cuda()
    dimg = img.cuda().view(n * Ti, Ew).contiguous()
    with torch.no_grad():
        pooled = bm.bert_forward_f32(st, "text_encoder.", cfg, dids, key_len, dimg, Ti)
        rows = bm.bert_forward_f32(st, "text_encoder.", cfg, dids, key_len, dimg, Ti, pool=False)
        text_rows = bm.bert_forward_f32(st, "text_encoder.", cfg, dids, key_len, None, 0, cross=False, pool=False)

    def oracle(dtype, enc=True, pick=1):
        out = bo.bert_forward(_cast(sd, dtype), ids, mask, img.to(dtype) if enc else None, cfg)
        return out[1] if pick else out[0][:, 0]

    _gate("g6 MED BERT multimodal pooler_output", pooled, oracle, golden=z["pooler_output"])
    _gate("g6 MED BERT multimodal class row", rows, lambda dt: oracle(dt, pick=0), golden=z["last_hidden_state"][:, 0])
    _gate("g6 MED BERT text mode class row", text_rows, lambda dt: oracle(dt, enc=False, pick=0))


def test_g7_vit_tokens():
    from oracle import blip_oracle as bo
    from uniir_amd import blip_model as bm
    z = np.load(os.path.join(G, "g7_vit.npz"))
    vit_cfg = json.loads(str(z["cfg"]))
    med_cfg = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=1, vocab_size=64,
                   max_position_embeddings=32)
    model = tiny_model(med_cfg, vit_cfg).cuda().eval()
    sd = load_sub(model, z, "sd::", "visual_encoder.")
    sd = {k[len("visual_encoder."):]: v for k, v in sd.items()}
    model._sync()
    x = torch.from_numpy(z["x"])
    with torch.no_grad():
        tok, T = bm.vit_forward_f32(model._online, "visual_encoder.", model.vit_cfg, model.image_size, x.cuda())
    y = torch.from_numpy(z["y"])
    assert T == y.shape[1]
    _gate("g7 BLIP ViT tokens", tok.view(y.shape), lambda dt: bo.vit_forward(_cast(sd, dt), x.to(dt), model.vit_cfg), golden=y)


@pytest.mark.parametrize("score_fusion", [False, True], ids=["blip_ff", "blip_sf"])
def test_g8_embeddings_every_mask_combination(score_fusion):
    from oracle import blip_oracle as bo
    z = np.load(os.path.join(G, "g8s_blipsf.npz" if score_fusion else "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    model = _model(score_fusion, med_cfg, vit_cfg, int(z["embed_dim"]) if score_fusion else None)
    sd = {k[len("sd0::"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd0::")}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    model = model.cuda().eval()
    ids, mask, img = torch.from_numpy(z["s0_ids"]), torch.from_numpy(z["s0_mask"]), torch.from_numpy(z["s0_img"])
    full = {n: p.detach().cpu().float() for n, p in model.named_parameters()}
    txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    n = ids.shape[0]
    if not score_fusion:
        got = _encode(model, "fp32", txt, img.cuda())
        _gate("g8 BLIP_FF embeddings", got,
              lambda dt: bo.encode_multimodal_input(_cast(full, dt), ids, mask, img.to(dt), model.vit_cfg, model.med_cfg))
        batch = {"txt_batched": txt, "image_batched": img.cuda(), "did_list": list(range(n))}
        model.precision = "fp32"
        with torch.no_grad():          # through the reference surface, too
            e1, ids1 = model.encode_mbeir_batch(batch)
            e2, _ = model(batch, encode_mbeir_batch=True)
        assert torch.equal(e1, got) and torch.equal(e2, got) and ids1 == batch["did_list"]
        return
    ones, zeros = torch.ones(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64)
    combos = {"the golden's masks": (torch.from_numpy(z["s0_tmask"]), torch.from_numpy(z["s0_imask"])), "text only": (ones, zeros),
              "image only": (zeros, ones), "both": (ones, ones)}
    for what, (tm, im) in combos.items():
        got = _encode(model, "fp32", txt, img.cuda(), (tm.cuda(), im.cuda()))
        _gate(f"g8s BLIP_SF embeddings, {what}", got,
              lambda dt: bo.encode_multimodal_input_sf(_cast(full, dt), ids, mask, img.to(dt), tm.to(dt), im.to(dt), model.vit_cfg,
                                                       model.med_cfg))


VIT_384 = dict(img_size=384, patch_size=16, embed_dim=64, depth=1, num_heads=1, drop_path_rate=0.0)          # 577 tokens
MED_384 = dict(hidden_size=64, intermediate_size=128, num_attention_heads=1, num_hidden_layers=2, vocab_size=64,
               max_position_embeddings=32)
LENS = (1, 7, 20)


@pytest.mark.parametrize("score_fusion", [False, True], ids=["blip_ff", "blip_sf"])
def test_384_pixels_577_image_tokens_and_the_gate_tells_fp32_from_fp16(score_fusion):
    """cross-attention over 577 keys with key_len on the self-attention, the third 256-row pass of the ViT's attention; pack_text,
    pool_last_layer and vit_grad_ckpt change no bit on this path"""
    from oracle import blip_oracle as bo
    model = _model(score_fusion, MED_384, VIT_384, embed_dim=32 if score_fusion else None, seed=5).cuda().eval()
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, MED_384["vocab_size"], (3, L), generator=g)
    ids[:, 0] = 1
    mask = (torch.arange(L).unsqueeze(0) < torch.tensor(LENS).unsqueeze(1)).long()
    ids = ids * mask
    img = torch.randn(3, 3, 384, 384, generator=torch.Generator().manual_seed(11))
    full = {n: p.detach().cpu().float() for n, p in model.named_parameters()}
    txt = lambda: types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())          # noqa: E731
    if score_fusion:
        tm, im = torch.tensor([1, 0, 1]), torch.tensor([1, 1, 0])
        masks = (tm.cuda(), im.cuda())
        oracle = lambda dt: bo.encode_multimodal_input_sf(_cast(full, dt), ids, mask, img.to(dt), tm.to(dt), im.to(dt), model.vit_cfg,      # noqa: E731
                                                          model.med_cfg)
    else:
        masks = (None, None)
        oracle = lambda dt: bo.encode_multimodal_input(_cast(full, dt), ids, mask, img.to(dt), model.vit_cfg, model.med_cfg)      # noqa: E731
    got = _encode(model, "fp32", txt(), img.cuda(), masks)
    assert not got.requires_grad
    what = "384 pixels BLIP_SF" if score_fusion else "384 pixels BLIP_FF"
    e32, o64 = _gate(what, got, oracle)
    half = _encode(model, "fp16", txt(), img.cuda(), masks)
    eh = _maxdiff(half, o64)
    print(f"\nOBS {what}: fp16 error {eh:.3e} = {eh / e32:.1f} E32 (outside the gate by {eh / (FACTOR * e32):.1f}x, wanted {APART:.0f}x)")
    assert eh >= APART * FACTOR * e32, (eh, e32)
    for pack, pool_last, boundary in ((False, False, 1), (True, True, 0)):
        model.pack_text, model.pool_last_layer, model.vit_recompute_from = pack, pool_last, boundary
        assert torch.equal(_encode(model, "fp32", txt(), img.cuda(), masks), got), (pack, pool_last, boundary)
        assert model.last_text_rows == (3 * L, 3 * L)          # the dense rows, whatever pack_text says
    assert model._online.h16_buf is not None          # fp16 built its shadow; fp32 reads the masters and builds none:
    fresh = _model(score_fusion, MED_384, VIT_384, embed_dim=32 if score_fusion else None, seed=5).cuda().eval()
    assert torch.equal(_encode(fresh, "fp32", txt(), img.cuda(), masks), got) and fresh._online.h16_buf is None and fresh._online.half_bytes() == 0


def test_guards_on_the_device_and_the_bf16_path_is_untouched():
    z = np.load(os.path.join(G, "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    model = _model(False, med_cfg, vit_cfg).cuda().eval()
    txt = types.SimpleNamespace(input_ids=torch.from_numpy(z["s0_ids"]).cuda(), attention_mask=torch.from_numpy(z["s0_mask"]).cuda())
    img = torch.from_numpy(z["s0_img"]).cuda()
    emb0 = _encode(model, "bf16", txt, img)
    model.precision, model.embed_fp32 = "fp32", False
    with pytest.raises(RuntimeError, match="unknown precision 'fp32'"), torch.no_grad():          # a module that has not opted in
        model.encode_multimodal_input(txt, img)
    model.embed_fp32 = True
    with pytest.raises(RuntimeError, match="no_grad"):          # grad enabled
        model.encode_multimodal_input(txt, img)
    with pytest.raises(RuntimeError, match="online"), torch.no_grad():
        model.encode_multimodal_input(txt, img, use_momentum=True)
    model.train()
    with pytest.raises(RuntimeError, match="eval"), torch.no_grad():
        model.encode_multimodal_input(txt, img)
    model.eval()
    model.precision = "fp64"
    with pytest.raises(RuntimeError, match="unknown precision"), torch.no_grad():
        model.encode_multimodal_input(txt, img)
    model.precision = "bf16"
    f = _encode(model, "fp32", txt, img)
    assert not torch.equal(f, emb0) and torch.equal(_encode(model, "bf16", txt, img), emb0)
