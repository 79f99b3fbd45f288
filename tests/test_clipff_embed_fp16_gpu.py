"""The fp16 embedding forward of CLIP_FF (CLIPFeatureFusion.precision = "fp16": the towers without pooling, the T5 stack with the
relative bias and the RMS norm, all on fp16 operands from the two stores' fp16 shadows) against oracle/clipff_oracle.py in fp32, next
to the bf16 forward on the same inputs; the entry points it calls; the fp16 weight copies behind the fused AdamW, in-place edits and
load_state_dict; the guards; and the embedder's opt-in switch.

Two geometries: the small model of tests/test_clipff_gpu.py (resident attention kernel) and tiny-ff-336 of tests/test_clipff_336_gpu.py
(77 + 577 = 654 fused tokens, streaming kernel, 4 items), the latter with the q projections scaled by Q_GAIN and as the module draws
them (q_gain = 1: logits of standard deviation 8).

The bounds: rel_bf16 < 2e-2 is the gate of tests/test_clipff_gpu.py; rel_fp16 < 0.35 * rel_bf16 is the project's figure for "three more
mantissa bits" (tests/test_blip_vit_fp16_gpu.py has the derivation).  The CPU oracle itself under autocast gives a ratio of 0.12 - 0.13
at the 654-token geometry."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))

import test_clipff_336_gpu as T336  # noqa: E402
from test_clipff_gpu import _model as small_model, rel  # noqa: E402

RATIO = 0.35
SMALL_T5 = dict(d_model=128, num_heads=2, d_ff=256, num_layers=2, d_kv=64)
BF16_ENTRY_POINTS = ("uniir_attention_fwd", "uniir_attention_fwd_packed", "uniir_attention_fwd_ex", "uniir_attention_fwd_rows",
                     "uniir_attention_fwd_long", "uniir_attention_one_fwd", "uniir_onequery_fwd", "uniir_attention_rel_fwd",
                     "uniir_attention_rel_fwd_long", "uniir_rmsnorm_fwd")
T5_Q = "block.0.layer.0.SelfAttention.q.weight"


def _small(seed=5):
    """-> model (eval), the oracle's tower state dict, cfg, T5 cfg, a CPU batch of 8 items"""
    from oracle import clip_oracle as O
    cfg = O.tiny_config(embed_dim=128, transformer_width=128, transformer_heads=2)
    m, sd = small_model(cfg, SMALL_T5, seed=seed)
    m.embed_fp16 = False          # whatever the environment says: the tests set what they test
    return m.eval(), sd, cfg, SMALL_T5, O.synthetic_batch(cfg, 4, seed=23)


def _336(q_gain=T336.Q_GAIN, seed=5):
    m, sd, cfg = T336.build("cuda", seed=seed, q_gain=q_gain)
    m.embed_fp16 = False
    return m.eval(), sd, cfg, T336.T5_CFG, T336.batch_of(cfg)


def _oracle(m, sd, cfg, t5_cfg, batch):
    from oracle import clipff_oracle as FF
    with torch.no_grad():
        return FF.encode_multimodal_input({k: v.clone() for k, v in sd.items()}, T336.t5_state(m), cfg, t5_cfg, batch["txt_batched"],
                                          batch["image_batched"]).float()


def _encode(m, precision, txt, img):
    """encode_multimodal_input at `precision` under no_grad; the attribute goes back to what it was"""
    was = m.precision
    m.precision = precision
    try:
        with torch.no_grad():
            return m.encode_multimodal_input(txt, img).clone()
    finally:
        m.precision = was


def _both_against_the_oracle(m, txt, img, want, what):
    b, h = _encode(m, "bf16", txt, img), _encode(m, "fp16", txt, img)
    assert b.dtype == h.dtype == torch.float32 and tuple(b.shape) == tuple(h.shape) == tuple(want.shape) and not h.requires_grad
    assert bool(torch.isfinite(h).all())
    rb, rh = rel(b, want), rel(h, want)
    print(f"\nOBS {what} rel_bf16 {rb:.3e} rel_fp16 {rh:.3e} ratio {rh / rb:.3f}")
    assert rb < 2e-2, (what, rb)
    assert rh < RATIO * rb, (what, rh, rb)
    return h


@pytest.mark.parametrize("geometry", ["small", "336-q-gain", "336-unscaled-q"])
def test_fp16_embeddings_beat_bf16_against_the_oracle(geometry):
    m, sd, cfg, t5_cfg, batch = _small() if geometry == "small" else _336(T336.Q_GAIN if geometry == "336-q-gain" else 1.0)
    want = _oracle(m, sd, cfg, t5_cfg, batch)
    txt, img = batch["txt_batched"].cuda(), batch["image_batched"].cuda()
    h = _both_against_the_oracle(m, txt, img, want, geometry)
    # through the reference surface, too: encode_mbeir_batch and forward(encode_mbeir_batch=True) are the same forward
    dbatch = {"txt_batched": txt, "image_batched": img, "txt_mask_batched": None, "image_mask_batched": None,
              "did_list": list(range(img.shape[0]))}
    m.precision = "fp16"
    with torch.no_grad():
        e1, ids1 = m.encode_mbeir_batch(dbatch)
        e2, ids2 = m(dbatch, encode_mbeir_batch=True)
    assert torch.equal(e1, h) and torch.equal(e2, h) and ids1 == ids2 == dbatch["did_list"]


@pytest.mark.parametrize("geometry", ["small", "336"])
def test_the_entry_points_the_fp16_forward_calls(geometry, monkeypatch):
    """one uniir_attn_rel_fwd*_f16 call per T5 layer with (items, fused tokens, heads) -- the resident entry point up to 512 tokens, the
    streaming one above -- and none to a bf16 attention entry point, to uniir_attention_rel_fwd* or to uniir_rmsnorm_fwd"""
    from uniir_amd import _lib
    m, sd, cfg, t5_cfg, batch = _small() if geometry == "small" else _336()
    txt, img = batch["txt_batched"].cuda(), batch["image_batched"].cuda()
    M = img.shape[0]
    T = cfg["context_length"] + (cfg["image_resolution"] // cfg["vision_patch_size"]) ** 2 + 1
    assert (T <= 512) == (geometry == "small") and (geometry == "small" or T == 654)
    want_h = _encode(m, "fp16", txt, img)          # before anything is replaced
    lib = _lib.load()
    seen, rms16, refused = [], [], []

    def counting(name, sink, pick):
        real = getattr(lib, name)

        def f(*a):
            sink.append((name,) + pick(a))
            return real(*a)
        monkeypatch.setattr(lib, name, f)

    for name in ("uniir_attn_rel_fwd_f16", "uniir_attn_rel_fwd_long_f16"):
        counting(name, seen, lambda a: tuple(a[7:10]))
    counting("uniir_rmsnorm_fwd_f16", rms16, lambda a: tuple(a[5:7]))
    for name in BF16_ENTRY_POINTS:
        def refuse(*a, _name=name):
            refused.append(_name)
            return -1
        monkeypatch.setattr(lib, name, refuse)
    got = _encode(m, "fp16", txt, img)
    entry = "uniir_attn_rel_fwd_f16" if T <= 512 else "uniir_attn_rel_fwd_long_f16"
    assert seen == [(entry, M, T, t5_cfg["num_heads"])] * t5_cfg["num_layers"], seen
    assert rms16 == [("uniir_rmsnorm_fwd_f16", M * T, t5_cfg["d_model"])] * (2 * t5_cfg["num_layers"] + 1), rms16
    assert not refused, refused
    assert torch.equal(got, want_h)
    with pytest.raises(RuntimeError):          # the stand-ins do refuse: the bf16 forward needs what they replaced
        _encode(m, "bf16", txt, img)
    assert refused


def test_the_fp16_copies_of_both_stores_follow_the_fused_adamw_in_place_edits_and_load_state_dict():
    """one bf16 training step with the project's AdamW (which writes the master weights and the bf16 shadows itself, the T5 group's
    too), then fp16 embeddings: those of a freshly built model that loaded the stepped state_dict, bit for bit -- and again after an
    in-place edit of a T5 and of a CLIP parameter, and after load_state_dict into a model whose fp16 copies already existed"""
    from uniir_amd.trainer import NativeAdamW
    m, sd, cfg, t5_cfg, batch = _small()
    dbatch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    txt, img = dbatch["txt_batched"], dbatch["image_batched"]
    before = _encode(m, "fp16", txt, img)          # the fp16 copies exist BEFORE the weights move
    assert m.clip_model._flat.h16_buf is not None and m._t5.h16_buf is not None
    opt = NativeAdamW(m.clip_model, lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, allreduce=False,
                      extra=[m.t5_optimizer_group(lr=1e-2)])
    m.train()
    opt.zero_grad()
    m(dbatch)["loss"].backward()
    t5_before, clip_before = m.t5_layers.get_parameter(T5_Q).detach().clone(), m.clip_model.visual.proj.detach().clone()
    opt.step()
    m.eval()
    assert not torch.equal(m.t5_layers.get_parameter(T5_Q), t5_before) and not torch.equal(m.clip_model.visual.proj, clip_before)
    got = _encode(m, "fp16", txt, img)
    assert not torch.equal(got, before)

    def fresh(seed):
        f = _small(seed=seed)[0]
        f.load_state_dict(m.state_dict())
        return f

    assert torch.equal(got, _encode(fresh(9), "fp16", txt, img))
    with torch.no_grad():          # a T5 parameter alone, then a CLIP parameter alone
        m.t5_layers.get_parameter("block.1.layer.1.DenseReluDense.wi.weight").mul_(1.25)
    got_t5 = _encode(m, "fp16", txt, img)
    assert not torch.equal(got_t5, got) and torch.equal(got_t5, _encode(fresh(10), "fp16", txt, img))
    with torch.no_grad():
        m.clip_model.get_parameter("transformer.resblocks.0.mlp.c_fc.weight").mul_(0.75)
        m.clip_model.visual.conv1.weight.mul_(1.5)          # the fp16 patch-embedding copy is no part of the store's shadow
    got_clip = _encode(m, "fp16", txt, img)
    assert not torch.equal(got_clip, got_t5) and torch.equal(got_clip, _encode(fresh(11), "fp16", txt, img))
    other = _small(seed=12)[0]          # its fp16 copies exist, of other weights
    assert not torch.equal(_encode(other, "fp16", txt, img), got_clip)
    other.load_state_dict(m.state_dict())
    assert torch.equal(_encode(other, "fp16", txt, img), got_clip)


def test_guards_and_the_bf16_path_is_untouched():
    m, sd, cfg, t5_cfg, batch = _small()
    dbatch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    txt, img = dbatch["txt_batched"], dbatch["image_batched"]
    emb0 = _encode(m, "bf16", txt, img)
    assert m.clip_model._flat.h16_buf is None and m._t5.h16_buf is None          # bf16 users allocate nothing
    assert m.clip_model._flat.half_bytes() == 0 and m._t5.half_bytes() == 0          # ... no fp16 padded copy either
    m.precision = "fp16"
    m.train()
    with pytest.raises(RuntimeError, match="eval"), torch.no_grad():
        m.encode_multimodal_input(txt, img)
    with pytest.raises(RuntimeError, match="eval"):
        m(dbatch)
    m.eval()
    with pytest.raises(RuntimeError, match="no_grad"):          # grad enabled
        m.encode_multimodal_input(txt, img)
    for bad in ("fp32", "half"):
        m.precision = bad
        with pytest.raises(RuntimeError, match="unknown precision"), torch.no_grad():
            m.encode_multimodal_input(txt, img)
    m.precision = "bf16"
    h = _encode(m, "fp16", txt, img)
    assert not torch.equal(h, emb0)
    # after fp16 was used and refused: the bf16 embeddings are what they were, bit for bit, and a bf16 training step still runs
    assert torch.equal(_encode(m, "bf16", txt, img), emb0)
    m.train()
    m.zero_grad()
    out = m(dbatch)
    out["loss"].backward()
    assert bool(torch.isfinite(out["loss"])) and float(m.t5_layers.get_parameter(T5_Q).grad.abs().max()) > 0


def _embedder():
    src = os.path.join(ROOT, "uniir_amd", "src")
    for p in (src, os.path.join(src, "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import mbeir_embedder
    return mbeir_embedder


def test_the_embedder_takes_the_fp16_forward_only_when_the_model_opted_in():
    E = _embedder()
    m, sd, cfg, t5_cfg, batch = _small(seed=4)
    txt, img = batch["txt_batched"], batch["image_batched"]
    cuts = ((0, 3), (3, 6), (6, 8))          # three batches, the last one smaller

    def loader():
        return [{"txt_batched": txt[a:b].clone(), "image_batched": img[a:b].clone(), "txt_mask_batched": None,
                 "image_mask_batched": None, "did_list": list(range(a, b))} for a, b in cuts]

    def direct(precision):
        return torch.cat([_encode(m, precision, b["txt_batched"].cuda(), b["image_batched"].cuda()) for b in loader()]).half()

    want_b, want_h = direct("bf16"), direct("fp16")
    assert not torch.equal(want_b, want_h)
    for embed_fp16, use_fp16, want in ((False, True, want_b), (False, False, want_b), (True, False, want_b), (True, True, want_h)):
        m.embed_fp16 = embed_fp16
        emb, id_list = E.generate_embeds_and_ids_on_device(m, loader(), "cuda:0", use_fp16=use_fp16)
        assert emb.dtype == torch.float16 and emb.is_cuda and id_list == list(range(8))
        assert torch.equal(emb, want), (embed_fp16, use_fp16)
        assert m.precision == "bf16" and m.clip_model.precision == "bf16"
