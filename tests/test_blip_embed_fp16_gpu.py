"""The fp16 embedding forward of BLIP_FF and BLIP_SF (BLIPFeatureFusion.precision = "fp16": ViT -> MED BERT -> pooler, or -> class row
-> projections -> fused sum, all on fp16 operands from the online store's fp16 shadow) against oracle/blip_oracle.py in fp32, next to
the bf16 forward on the same inputs; the bitwise equalities the bf16 forward has (pack_text, pool_last_layer) in fp16; the fp16 weight
copies behind the fused AdamW and in-place edits; the guards; and the embedder's opt-in switch.

The bounds: rel_bf16 < 2e-2 is that of tests/test_blip_gpu.py; rel_fp16 < 0.35 * rel_bf16 is the project's figure for "three more
mantissa bits" (tests/test_blip_vit_fp16_gpu.py has the derivation, tests/test_fp32_parity_gpu.py asserts it for the CLIP towers)."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATIO = 0.35
L = 20
LENS = (1, 7, 20)
BF16_ATTENTION = ("uniir_attention_fwd", "uniir_attention_fwd_packed", "uniir_attention_fwd_ex", "uniir_attention_fwd_rows",
                  "uniir_attention_fwd_long", "uniir_attention_one_fwd", "uniir_onequery_fwd")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def _model(score_fusion, med_cfg, vit_cfg, embed_dim=None, seed=0):
    from uniir_amd import blip_model as bm
    cls = bm.BLIPScoreFusion if score_fusion else bm.BLIPFeatureFusion
    m = cls(med_config=med_cfg, vit_config=vit_cfg, embed_dim=embed_dim or med_cfg["hidden_size"], queue_size=16, momentum=0.9,
            config=types.SimpleNamespace(tokenizer_max_length=L), seed=seed)
    m.pool_last_layer, m.embed_fp16 = False, False          # whatever the environment says: the tests set what they test
    return m


def _golden(score_fusion):
    """model with the golden's weights, its first batch, and the oracle's fp32 embeddings of that batch"""
    from oracle import blip_oracle as bo
    z = np.load(os.path.join(G, "g8s_blipsf.npz" if score_fusion else "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    model = _model(score_fusion, med_cfg, vit_cfg, int(z["embed_dim"]) if score_fusion else None)
    sd = {k[len("sd0::"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd0::")}
    assert not model.load_state_dict(sd, strict=False).unexpected_keys
    model = model.cuda().eval()
    ids, mask, img = torch.from_numpy(z["s0_ids"]), torch.from_numpy(z["s0_mask"]), torch.from_numpy(z["s0_img"])
    full = {n: p.detach().cpu().float() for n, p in model.named_parameters()}
    with torch.no_grad():
        if score_fusion:
            tm, im = torch.from_numpy(z["s0_tmask"]), torch.from_numpy(z["s0_imask"])
            want = bo.encode_multimodal_input_sf(full, ids, mask, img, tm.float(), im.float(), model.vit_cfg, model.med_cfg)
            masks = (tm.cuda(), im.cuda())
        else:
            want = bo.encode_multimodal_input(full, ids, mask, img, model.vit_cfg, model.med_cfg)
            masks = (None, None)
    txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    return model, txt, img.cuda(), masks, want


def _encode(model, precision, txt, img, masks=(None, None)):
    """encode_multimodal_input at `precision`; the attribute goes back to what it was"""
    was = model.precision
    model.precision = precision
    try:
        with torch.no_grad():
            return model.encode_multimodal_input(txt, img, *masks).clone()
    finally:
        model.precision = was


def _both_against_the_oracle(model, txt, img, masks, want, what):
    b, h = _encode(model, "bf16", txt, img, masks), _encode(model, "fp16", txt, img, masks)
    assert b.dtype == h.dtype == torch.float32 and b.shape == h.shape == want.shape and not h.requires_grad
    rb, rh = rel(b, want), rel(h, want)
    print(f"\nOBS {what} rel_bf16 {rb:.3e} rel_fp16 {rh:.3e} ratio {rh / rb:.3f}")
    assert rb < 2e-2, (what, rb)
    assert rh < RATIO * rb, (what, rh, rb)


@pytest.mark.parametrize("score_fusion", [False, True], ids=["blip_ff", "blip_sf"])
def test_fp16_embeddings_beat_bf16_against_the_oracle(score_fusion):
    model, txt, img, masks, want = _golden(score_fusion)
    _both_against_the_oracle(model, txt, img, masks, want, "g8s BLIP_SF" if score_fusion else "g8 BLIP_FF")
    # through the reference surface, too: encode_mbeir_batch and forward(encode_mbeir_batch=True) are the same forward
    batch = {"txt_batched": txt, "image_batched": img, "txt_mask_batched": masks[0], "image_mask_batched": masks[1],
             "did_list": list(range(img.shape[0]))}
    model.precision = "fp16"
    h = _encode(model, "fp16", txt, img, masks)
    with torch.no_grad():
        e1, ids1 = model.encode_mbeir_batch(batch)
        e2, ids2 = model(batch, encode_mbeir_batch=True)
    assert torch.equal(e1, h) and torch.equal(e2, h) and ids1 == ids2 == batch["did_list"]


def _captions(vocab, M=3, seed=7):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab, (M, L), generator=g)
    ids[:, 0] = 1
    mask = (torch.arange(L).unsqueeze(0) < torch.tensor(LENS[:M]).unsqueeze(1)).long()
    return ids * mask, mask


VIT_384 = dict(img_size=384, patch_size=16, embed_dim=128, depth=1, num_heads=2, drop_path_rate=0.0)          # 577 tokens
MED_384 = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=1, vocab_size=64,
               max_position_embeddings=32)


def test_384_pixels_fp16_against_the_oracle_and_the_attention_calls_it_makes(monkeypatch):
    """577 image tokens: per BERT layer one self-attention call (20 x 20) and one cross-attention call (20 x 577, the streaming fp16
    kernel) through uniir_attn_general_fwd_f16, and no bf16 attention entry point"""
    from oracle import blip_oracle as bo
    from uniir_amd import _lib
    model = _model(False, MED_384, VIT_384, seed=5).cuda().eval()
    ids, mask = _captions(MED_384["vocab_size"])
    img = torch.randn(3, 3, 384, 384, generator=torch.Generator().manual_seed(11))
    full = {n: p.detach().cpu().float() for n, p in model.named_parameters()}
    with torch.no_grad():
        want = bo.encode_multimodal_input(full, ids, mask, img, model.vit_cfg, model.med_cfg)
    txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    _both_against_the_oracle(model, txt, img.cuda(), (None, None), want, "384 pixels")
    lib = _lib.load()
    real, seen, bf16_calls = lib.uniir_attn_general_fwd_f16, [], []

    def counted(q, q_ld, k, v, kv_ld, out, out_ld, lse, row_off, kv_packed, key_len, batch, tq, tk, heads, stream):
        seen.append((batch, tq, tk, heads))
        return real(q, q_ld, k, v, kv_ld, out, out_ld, lse, row_off, kv_packed, key_len, batch, tq, tk, heads, stream)

    monkeypatch.setattr(lib, "uniir_attn_general_fwd_f16", counted)
    for name in BF16_ATTENTION:
        def refuse(*a, _name=name):
            bf16_calls.append(_name)
            return -1
        monkeypatch.setattr(lib, name, refuse)
    for pack in (True, False):
        model.pack_text = pack
        del seen[:]
        _encode(model, "fp16", types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda()), img.cuda())
        assert seen == [(3, L, L, 2), (3, L, 577, 2)] * MED_384["num_hidden_layers"], (pack, seen)
    assert not bf16_calls, bf16_calls


@pytest.mark.parametrize("score_fusion", [False, True], ids=["blip_ff", "blip_sf"])
def test_pack_text_and_pool_last_layer_change_no_bit_in_fp16(score_fusion):
    z = np.load(os.path.join(G, "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    model = _model(score_fusion, med_cfg, vit_cfg, seed=3).cuda().eval()
    ids, mask = _captions(med_cfg["vocab_size"])
    img = torch.randn(3, 3, vit_cfg["img_size"], vit_cfg["img_size"], generator=torch.Generator().manual_seed(2)).cuda()

    def run(pack, pool_last):
        model.pack_text, model.pool_last_layer = pack, pool_last
        del model.path_log[:]
        txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())          # fresh tensors: no remembered pack
        e = _encode(model, "fp16", txt, img)
        assert model.last_text_rows == ((sum(LENS) if pack else 3 * L), 3 * L)
        assert len(model.path_log) == int(pool_last)
        return e

    base = run(False, False)
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    for pack, pool_last in ((True, False), (False, True), (True, True)):
        e = run(pack, pool_last)
        assert torch.equal(e, base), (pack, pool_last, float((e - base).abs().max()))
    model.pack_text, model.pool_last_layer = True, False
    assert not torch.equal(_encode(model, "bf16", types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda()), img), base)


def _g8_batch(z):
    b = len(z["s0_pdid"])
    return {"txt_batched": types.SimpleNamespace(input_ids=torch.from_numpy(z["s0_ids"]).cuda(),
                                                 attention_mask=torch.from_numpy(z["s0_mask"]).cuda()),
            "image_batched": torch.from_numpy(z["s0_img"]).cuda(), "p_did_list": torch.from_numpy(z["s0_pdid"]),
            "index_mapping": {"query": [[2 * i] for i in range(b)], "pos_cand": [[2 * i + 1] for i in range(b)]}}


def test_the_fp16_copies_of_berts_weights_follow_the_fused_adamw_and_in_place_edits():
    """one bf16 training step with the project's AdamW (which writes the master weights and the bf16 shadow itself), then fp16
    embeddings: those of a fresh model that loaded the stepped state_dict, bit for bit -- and again after in-place edits of BERT's
    weights (a spanning q | k | v tensor, a cross k | v tensor and the pooler among them)"""
    from uniir_amd.trainer import NativeAdamW
    z = np.load(os.path.join(G, "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    batch = _g8_batch(z)
    txt, img = batch["txt_batched"], batch["image_batched"]
    model = _model(False, med_cfg, vit_cfg).cuda().eval()
    before = _encode(model, "fp16", txt, img)          # the fp16 copies exist BEFORE the weights move
    model.train()
    opt = NativeAdamW(model, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, allreduce=False)
    opt.zero_grad()
    model(batch, alpha=0.4)["loss"].backward()
    opt.step()
    model.eval()
    got = _encode(model, "fp16", txt, img)
    assert not torch.equal(got, before)

    def fresh():
        m = _model(False, med_cfg, vit_cfg, seed=9).cuda().eval()
        m.load_state_dict(model.state_dict())
        return _encode(m, "fp16", txt, img)

    assert torch.equal(got, fresh())
    with torch.no_grad():
        model.get_parameter("text_encoder.encoder.layer.0.attention.self.key.weight")[3, :7] += 0.5
        model.get_parameter("text_encoder.encoder.layer.1.crossattention.self.value.weight")[5, :9] -= 0.25
        model.get_parameter("text_encoder.encoder.layer.1.intermediate.dense.weight")[1, :5] += 0.5
        model.get_parameter("text_encoder.pooler.dense.weight")[2, :11] -= 0.5
    got2 = _encode(model, "fp16", txt, img)
    assert not torch.equal(got2, got) and torch.equal(got2, fresh())
    model._momentum_update()          # the EMA kernel leaves the online copies valid and the result unchanged
    assert torch.equal(_encode(model, "fp16", txt, img), got2)


@pytest.mark.parametrize("score_fusion", [False, True], ids=["blip_ff", "blip_sf"])
def test_guards_and_the_bf16_path_is_untouched(score_fusion):
    z = np.load(os.path.join(G, "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    batch = _g8_batch(z)
    txt, img = batch["txt_batched"], batch["image_batched"]
    model = _model(score_fusion, med_cfg, vit_cfg).cuda().eval()
    emb0 = _encode(model, "bf16", txt, img)
    assert model._online.h16_buf is None and model._online.half_bytes() == 0          # bf16 users allocate nothing
    model.precision = "fp16"
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.encode_multimodal_input(txt, img)
    with pytest.raises(RuntimeError, match="eval"):
        model(batch, alpha=0.4)
    model.eval()
    with pytest.raises(RuntimeError, match="online"):
        model.encode_multimodal_input(txt, img, use_momentum=True)
    model.precision = "fp32"
    with pytest.raises(RuntimeError, match="unknown precision"):
        model.encode_multimodal_input(txt, img)
    model.precision = "bf16"
    h = _encode(model, "fp16", txt, img)
    assert model._online.h16_buf is not None and model._mom.h16_buf is None and not torch.equal(h, emb0)
    # after fp16 was used and refused: the bf16 embeddings are what they were, bit for bit, and a bf16 training step still runs
    assert torch.equal(_encode(model, "bf16", txt, img), emb0)
    model.train()
    model.zero_grad()
    out = model(batch, alpha=0.4)
    out["loss"].backward()
    assert bool(torch.isfinite(out["loss"])) and float(model.get_parameter("text_encoder.embeddings.word_embeddings.weight").grad.abs().max()) > 0


def _embedder():
    src = os.path.join(ROOT, "uniir_amd", "src")
    for p in (src, os.path.join(src, "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import mbeir_embedder
    return mbeir_embedder


@pytest.mark.parametrize("score_fusion", [False, True], ids=["blip_ff", "blip_sf"])
def test_the_embedder_takes_the_fp16_forward_only_when_the_model_opted_in(score_fusion):
    E = _embedder()
    z = np.load(os.path.join(G, "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    model = _model(score_fusion, med_cfg, vit_cfg, seed=4).cuda().eval()
    ids, mask, img = torch.from_numpy(z["s0_ids"]), torch.from_numpy(z["s0_mask"]), torch.from_numpy(z["s0_img"])
    cuts = ((0, 3), (3, 6), (6, 8))          # three batches, the last one smaller

    def loader():
        return [{"txt_batched": types.SimpleNamespace(input_ids=ids[a:b].cuda(), attention_mask=mask[a:b].cuda()),
                 "image_batched": img[a:b].clone(), "did_list": list(range(a, b))} for a, b in cuts]

    def direct(precision):
        return torch.cat([_encode(model, precision, b["txt_batched"], b["image_batched"].cuda()) for b in loader()]).half().cpu()

    want_b, want_h = direct("bf16"), direct("fp16")
    assert not torch.equal(want_b, want_h)
    for embed_fp16, use_fp16, want in ((False, True, want_b), (False, False, want_b), (True, False, want_b), (True, True, want_h)):
        model.embed_fp16 = embed_fp16
        emb, id_list = E.generate_embeds_and_ids_for_dataset_with_gather(model, loader(), "cuda:0", use_fp16=use_fp16)
        assert emb.dtype == np.float16 and id_list == list(range(8))
        assert torch.equal(torch.from_numpy(emb), want), (embed_fp16, use_fp16)
        assert model.precision == "bf16"
