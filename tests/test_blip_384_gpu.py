"""BLIP_FF at 384 pixels: 577 image tokens under the MED cross-attention, the key count of the reference's second BLIP class
(backbone/blip.py, image_size = 384) -- above the 512 keys of the resident attention kernels, so the cross-attention of every BERT layer
runs uniir_attention_fwd_long / _bwd_long (csrc/attention_long.hip) and the ViT the plain 577-token kernels.  A tiny model with the real
token geometry (patch 16, 24 x 24 patches + class token) against oracle/blip_oracle.py, with the gates the existing BLIP tests
(tests/test_blip_gpu.py, tests/test_recompute_towers_gpu.py) put on the same quantities: the arithmetic is the same, the key rows are
longer.  Captions of 12 positions with valid lengths 12, 1 and ragged ones; 4 items (2 pairs)."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

L, M = 12, 4
VIT = dict(img_size=384, patch_size=16, embed_dim=128, depth=2, num_heads=2)           # 577 tokens
MED = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=2, vocab_size=64,
           max_position_embeddings=32)
VALID = (12, 1, 7, 5)
GRADS = ("visual_encoder.blocks.0.attn.qkv.weight", "visual_encoder.blocks.1.mlp.fc2.weight", "visual_encoder.pos_embed",
         "visual_encoder.patch_embed.proj.weight", "text_encoder.embeddings.word_embeddings.weight",
         "text_encoder.encoder.layer.0.attention.self.query.weight",
         "text_encoder.encoder.layer.0.crossattention.self.key.weight",
         "text_encoder.encoder.layer.1.crossattention.self.value.weight",
         "text_encoder.encoder.layer.1.output.dense.weight", "text_encoder.pooler.dense.weight")


def rel(a, b):
    a, b = torch.as_tensor(a).double().cpu().flatten(), torch.as_tensor(b).double().cpu().flatten()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def tiny_model(med=MED, vit=VIT, seed=3, gain=1.0, **kw):
    """gain: factor on every weight matrix and embedding table (online and momentum copies alike), see BASE_GAIN"""
    from uniir_amd.blip_model import BLIPFeatureFusion
    model = BLIPFeatureFusion(med_config=med, vit_config=vit, embed_dim=med["hidden_size"], queue_size=16, momentum=0.995,
                              config=types.SimpleNamespace(tokenizer_max_length=L), seed=seed, **kw)
    if gain != 1.0:
        with torch.no_grad():
            for n, p in model.named_parameters():
                if p.dim() >= 2 and "norm" not in n.lower():
                    p.mul_(gain)
    return model


# The model draws its matrices at std 0.02 whatever the width.  A 128-wide projection then has a gain of 0.02 * sqrt(128) = 0.23
# where BERT-base's 768-wide one has 0.55, so the sublayers barely move the residual stream, every item's pooled [ENC] state is
# nearly the same vector (cosines 0.9975 .. 0.9996 between the items of this batch in the fp32 oracle) and the contrastive loss is
# a function of differences of about 3 % of the embeddings' length: the bf16 rounding of the activations (2^-9 per operand) is then
# 10 % of the signal.  The oracle itself under torch.autocast("cpu", bfloat16) shows it, with no kernel of this project involved
# (tests/test_blip_384_ref.py asserts it on the CPU): its gradients are 4 % .. 25 % away from its own fp32 gradients at gain 1 and
# 1.5 % .. 2.7 % at the gain below.  The contrastive test therefore
# draws the matrices at the per-projection gain of the 768-wide model, sqrt(768 / 128) = 2.45 -> 2.5 (cosines 0.93 .. 0.98); the
# tests whose loss is a fixed linear functional of the embedding keep the model's own initialisation.
BASE_GAIN = 2.5


def _inputs():
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, MED["vocab_size"], (M, L), generator=g)
    ids[:, 0] = 1
    mask = (torch.arange(L).unsqueeze(0) < torch.tensor(VALID).unsqueeze(1)).long()
    return ids * mask, mask, torch.randn(M, 3, 384, 384, generator=g)


def _batch(ids, mask, img):
    pairs = M // 2
    return {"txt_batched": types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda()), "image_batched": img.cuda(),
            "p_did_list": torch.tensor([501, 502]),
            "index_mapping": {"query": [[2 * i] for i in range(pairs)], "pos_cand": [[2 * i + 1] for i in range(pairs)]}}


def _oracle_step(sd, ids, mask, img, state, vit_cfg, med_cfg):
    """one contrastive step of the oracle on `sd` (online fp32 entries get gradients) -> its outputs"""
    from oracle import blip_oracle as bo
    for n in sd:
        if sd[n].dtype == torch.float32 and "_m." not in n:
            sd[n].requires_grad_(True)
    out = bo.contrastive_loss(sd, state, {"ids": ids, "mask": mask, "img": img,
                                          "index_mapping": {"query": [[0], [2]], "pos_cand": [[1], [3]]},
                                          "p_did_list": torch.tensor([501, 502])}, 0.4, vit_cfg, med_cfg, 0.995)
    out["loss"].backward()
    return out


def _queues(K):
    g = torch.Generator().manual_seed(9)
    return (torch.nn.functional.normalize(torch.randn(128, K, generator=g), dim=0),
            torch.nn.functional.normalize(torch.randn(128, K, generator=g), dim=0), torch.arange(900, 900 + K).view(1, K))


def _device_against_oracle(gain):
    """eval-mode embedding and one training step of the device model against the oracle at the given weight gain -> the figures"""
    from oracle import blip_oracle as bo
    torch.manual_seed(0)
    model = tiny_model(gain=gain).cuda()
    model.eval()
    ids, mask, img = _inputs()
    qq, cq, iq = _queues(model.queue_size)
    with torch.no_grad():
        model.query_queue.copy_(qq.cuda())
        model.cand_queue.copy_(cq.cuda())
        model.idx_queue.copy_(iq.cuda())
    sd = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    batch = _batch(ids, mask, img)
    with torch.no_grad():
        emb = model.encode_multimodal_input(batch["txt_batched"], batch["image_batched"])
        ref = bo.encode_multimodal_input(sd, ids, mask, img, model.vit_cfg, model.med_cfg)
    state = {"query_queue": qq.clone(), "cand_queue": cq.clone(), "idx_queue": iq.clone(), "ptr": int(model.new_ptr_queue.item())}
    out_o = _oracle_step(sd, ids, mask, img, state, model.vit_cfg, model.med_cfg)
    model.zero_grad()
    out_d = model(batch, alpha=0.4)
    out_d["loss"].backward()
    return dict(emb=rel(emb, ref), loss=(out_d["loss"].item(), out_o["loss"].item()),
                acc=(out_d["accuracy"].item(), out_o["accuracy"].item()),
                idx_equal=np.array_equal(model.idx_queue.cpu().numpy(), state["idx_queue"].numpy()),
                queue=rel(model.query_queue, state["query_queue"]),
                grads={n: rel(model.get_parameter(n).grad, sd[n].grad) for n in GRADS}, temp=rel(model.temp.grad, sd["temp"].grad))


def test_blip_ff_384_embedding_and_training_step_against_the_oracle():
    """eval mode: encode_multimodal_input against the oracle, then one training step (momentum encoders, queue) against
    contrastive_loss: loss, accuracy, d temp and sampled parameter gradients -- the cross-attention key / value projections, whose
    gradients come out of dk / dv of the 577-key backward, and the ViT position embedding among them.  Judged at BASE_GAIN; the
    same figures at the model's own initialisation (gain 1) are printed, not judged: see BASE_GAIN and tests/test_blip_384_ref.py."""
    r1 = _device_against_oracle(1.0)
    print("\nOBS blip-384 gain 1.0 (not judged) emb rel", r1["emb"], "loss", r1["loss"], "temp", round(r1["temp"], 4), "grad rel",
          {k[-40:]: round(v, 4) for k, v in r1["grads"].items()})
    r = _device_against_oracle(BASE_GAIN)
    print("OBS blip-384 gain", BASE_GAIN, "emb rel", r["emb"], "loss", r["loss"], "temp", round(r["temp"], 4), "grad rel",
          {k[-40:]: round(v, 4) for k, v in r["grads"].items()})
    assert r["emb"] < 2e-2
    assert abs(r["loss"][0] - r["loss"][1]) < 2e-2 * max(1.0, abs(r["loss"][1]))
    assert r["acc"][0] == r["acc"][1]
    assert r["idx_equal"]
    assert r["queue"] < 2e-2
    assert max(r["grads"].values()) < 8e-2, r["grads"]
    assert r["temp"] < 8e-2


def test_blip_ff_384_train_mode_dropout_matches_the_masked_oracle():
    """train mode with attention dropout 0.2, hidden dropout 0.1 and DropPath: the counter-based masks are exported
    (uniir_dropout_mask, the same seeds in the same order) into the oracle's mask hooks.  The cross-attention masks are [M][H][L][577]:
    a dropout coordinate taken with another tk, or at the packed row numbers, would not match them."""
    from oracle import blip_oracle as bo
    from uniir_amd import ops
    med = dict(MED, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.2)
    vit = dict(VIT, drop_path_rate=0.5)
    model = tiny_model(med, vit).cuda()
    assert model.pack_text
    sd = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    ids, mask, img = _inputs()
    txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    model.eval()
    with torch.no_grad():
        e0 = model.encode_multimodal_input(txt, img.cuda())
    ref_eval = bo.encode_multimodal_input(sd, ids, mask, img, model.vit_cfg, model.med_cfg)
    assert rel(e0, ref_eval) < 2e-2
    model.train()
    model.zero_grad()
    torch.manual_seed(5)
    emb = model.encode_multimodal_input(txt, img.cuda())
    assert rel(emb, ref_eval) > 5e-2          # the masks did something
    w = torch.randn(emb.shape, generator=torch.Generator().manual_seed(1))
    (emb * w.cuda()).sum().backward()
    torch.manual_seed(5)                      # the same draws, replayed for the oracle
    seeds = ops.DropSeeds()
    depth = vit["depth"]
    keep = 1.0 - torch.linspace(0, 0.5, depth).view(depth, 1, 1)
    rowscale = torch.floor(keep + torch.rand(depth, 2, M)) / keep
    path_iter = iter([rowscale[i, j] for i in range(depth) for j in range(2)])
    shapes = []

    def masks(kind, shape):
        if kind == "path":
            return next(path_iter).view(shape)
        shapes.append(tuple(shape))
        p = med["hidden_dropout_prob"] if kind == "hidden" else med["attention_probs_dropout_prob"]
        buf = torch.empty(int(np.prod(shape)), device="cuda")
        ops.call("uniir_dropout_mask", buf, buf.numel(), p, seeds.next())
        return buf.view(*shape).cpu()

    sdg = {k: v.clone().requires_grad_(v.dtype == torch.float32) for k, v in sd.items()}
    tok = bo.vit_forward(sdg, img, model.vit_cfg, prefix="visual_encoder.", masks=masks)
    assert tok.shape[1] == 577
    ref = bo.bert_forward(sdg, ids, mask, tok, model.med_cfg, prefix="text_encoder.", masks=masks)[1]
    assert (M, 2, L, 577) in shapes          # the cross-attention masks of the long kernels
    print("OBS blip-384 train emb rel", rel(emb, ref))
    assert rel(emb, ref) < 2e-2, rel(emb, ref)
    (ref * w).sum().backward()
    errs = {}
    for name in ("visual_encoder.blocks.0.attn.qkv.weight", "visual_encoder.blocks.0.attn.proj.bias",
                 "visual_encoder.blocks.1.mlp.fc2.bias", "visual_encoder.pos_embed",
                 "text_encoder.embeddings.word_embeddings.weight", "text_encoder.encoder.layer.0.attention.self.query.weight",
                 "text_encoder.encoder.layer.0.crossattention.self.key.weight",
                 "text_encoder.encoder.layer.1.crossattention.self.value.weight",
                 "text_encoder.encoder.layer.0.attention.output.dense.bias",
                 "text_encoder.encoder.layer.1.output.dense.weight", "text_encoder.pooler.dense.weight"):
        errs[name] = rel(model.get_parameter(name).grad, sdg[name].grad)
    print("OBS blip-384 train grad rel", {k[-40:]: round(v, 4) for k, v in errs.items()})
    assert max(errs.values()) < 8e-2, errs


def test_blip_ff_384_packed_bert_rows_equal_the_padded_rows():
    """pack_text on == off at 577 image tokens: packed query rows (q_row_off) against the dense padded call of the same entry point.
    Embeddings bitwise in eval and train mode, online and momentum; parameter gradients up to the order of the fp32 additions in the
    weight-gradient reductions (2e-5 of the largest element, as in test_packed_bert_rows_equal_the_padded_rows)."""
    med = dict(MED, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    vit = dict(VIT, drop_path_rate=0.1)
    model = tiny_model(med, vit, seed=11).cuda()
    ids, mask, img = _inputs()
    img = img.cuda()
    w = torch.randn(M, model.embed_dim, generator=torch.Generator().manual_seed(3)).cuda()

    def run(pack, train):
        model.pack_text = pack
        model.train(train)
        model.zero_grad()
        txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())     # fresh tensors: no remembered pack
        torch.manual_seed(21)
        emb = model.encode_multimodal_input(txt, img)
        rows = model.last_text_rows
        (emb * w).sum().backward()
        grads = {n: p.grad.detach().clone() for n, p in model._online_params() if n not in model._frozen and n != "temp"}
        with torch.no_grad():
            torch.manual_seed(22)
            emb_m = model.encode_multimodal_input(txt, img, use_momentum=True)
        return emb.detach().clone(), emb_m.clone(), grads, rows

    for train in (False, True):
        e_d, m_d, g_d, rows_d = run(False, train)
        e_p, m_p, g_p, rows_p = run(True, train)
        assert rows_d == (M * L, M * L) and rows_p == (sum(VALID), M * L)
        assert torch.equal(e_p, e_d), (train, (e_p - e_d).abs().max().item())
        assert torch.equal(m_p, m_d), train
        worst = max((float((g_p[n] - g_d[n]).abs().max()) / (float(g_d[n].abs().max()) + 1e-12), n) for n in g_d)
        assert worst[0] <= 2e-5, (train, worst)
        assert all(float(g_d[n].abs().max()) > 0 for n in g_d if "crossattention" in n)


def _step(ckpt):
    med = dict(MED, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    vit = dict(VIT, drop_path_rate=0.1)
    model = tiny_model(med, vit, seed=9, vit_grad_ckpt=ckpt, vit_ckpt_layer=1).cuda()
    assert model.vit_recompute_from == (1 if ckpt else 2)
    model.train()
    torch.manual_seed(31)
    model.zero_grad()
    out = model(_batch(*_inputs()), alpha=0.3)
    out["loss"].backward()
    torch.cuda.synchronize()
    return dict(loss=float(out["loss"].detach()), emb=(model.query_queue.clone(), model.cand_queue.clone()),
                grads={n: p.grad.detach().clone() for n, p in model._online_params() if n not in model._frozen},
                g32=model._online.g32.clone(), mom=model._mom.p32.clone())


@pytest.fixture(scope="module")
def stored_step():
    return _step(False)


def _same_step(a, b, what):
    assert a["loss"] == b["loss"], (what, a["loss"], b["loss"])
    assert torch.equal(a["g32"], b["g32"]), (what, int((a["g32"] != b["g32"]).sum()))
    for n, g in b["grads"].items():
        assert torch.equal(a["grads"][n], g), (what, n)
    assert torch.equal(a["mom"], b["mom"]), what
    for x, y in zip(a["emb"], b["emb"]):          # the momentum embeddings the step put into the queues
        assert torch.equal(x, y), what


def test_blip_ff_384_training_step_is_reproducible_bit_for_bit(stored_step):
    """two identical training steps (train mode, dropout and DropPath on): loss, flat gradients, momentum weights and queues equal"""
    _same_step(_step(False), stored_step, "stored, repeated")
    assert float(stored_step["g32"].abs().max()) > 0


def test_blip_ff_384_step_with_vit_grad_ckpt_equals_the_stored_step(stored_step):
    """vit_grad_ckpt=True, vit_ckpt_layer=1 (block 1 of 2 recomputed at 577 tokens) against the stored step, as
    tests/test_recompute_towers_gpu.py compares them"""
    _same_step(_step(True), stored_step, "recomputed")


def test_checkpoint_of_224_pixels_loads_into_the_384_pixel_model(tmp_path):
    """blip_front.load_checkpoint resizes a 14 x 14 position grid to 24 x 24 (bicubic, class token kept) and the model then runs"""
    from uniir_amd.blip_front import interpolate_pos_embed, load_checkpoint
    small = tiny_model(vit=dict(VIT, img_size=224), seed=5)
    sd = {k: v.detach().clone() for k, v in small.state_dict().items()}
    assert sd["visual_encoder.pos_embed"].shape == (1, 197, 128)
    path = str(tmp_path / "blip224.pth")
    torch.save({"model": sd}, path)
    model, msg = load_checkpoint(tiny_model(seed=6), path)
    assert not msg.unexpected_keys and not msg.missing_keys, msg
    want = interpolate_pos_embed(sd["visual_encoder.pos_embed"], 576)
    assert want.shape == (1, 577, 128)
    assert torch.equal(model.visual_encoder.pos_embed.detach().cpu(), want)
    assert torch.equal(model.visual_encoder_m.pos_embed.detach().cpu(), interpolate_pos_embed(sd["visual_encoder_m.pos_embed"], 576))
    assert torch.equal(model.text_encoder.pooler.dense.weight.detach().cpu(), sd["text_encoder.pooler.dense.weight"])
    model = model.cuda().eval()
    ids, mask, img = _inputs()
    with torch.no_grad():
        emb = model.encode_multimodal_input(types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda()), img.cuda())
    assert emb.shape == (M, 128) and bool(torch.isfinite(emb).all())
