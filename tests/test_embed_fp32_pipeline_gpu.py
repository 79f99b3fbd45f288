"""use_fp16: False through the embedder (mbeir_embedder.generate_embeds_and_ids_for_dataset_with_gather) on one tiny model each of
CLIP_SF, BLIP_FF and CLIP_FF, a two-batch list loader: with embed_fp32 set the extraction is, bit for bit, the same loop run with
precision = "fp32" set by hand, and the precision is "bf16" again afterwards; with embed_fp32 off it is today's bf16 extraction bit for
bit.  What is stored -- fp16, in loader order -- does not change."""
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))

MED = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=2, vocab_size=64, max_position_embeddings=32)
VIT = dict(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, drop_path_rate=0.0)
CUTS = ((0, 3), (3, 4))          # two batches, the second smaller


def _embedder():
    src = os.path.join(ROOT, "uniir_amd", "src")
    for p in (src, os.path.join(src, "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import mbeir_embedder
    return mbeir_embedder


def _clip_batches(cfg):
    from oracle import clip_oracle as O
    b = O.synthetic_batch(cfg, 2, seed=23)
    return lambda: [{"txt_batched": b["txt_batched"][lo:hi].clone(), "image_batched": b["image_batched"][lo:hi].clone(),
                     "txt_mask_batched": b["txt_mask_batched"][lo:hi].clone(), "image_mask_batched": b["image_mask_batched"][lo:hi].clone(),
                     "did_list": list(range(lo, hi))} for lo, hi in CUTS]


def _clip_sf():
    from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
    from oracle import clip_oracle as O
    from uniir_amd import clip_model
    cfg = O.tiny_config()
    clip_model.CLIP_CONFIGS["tiny-sf"] = cfg
    config = types.SimpleNamespace(model=types.SimpleNamespace(gather_embeddings=False), data_config=types.SimpleNamespace(in_batch_neg_num=0))
    m = CLIPScoreFusion("tiny-sf", device="cuda", config=config)
    m.clip_model.load_state_dict(O.init_state_dict(cfg, seed=3), strict=True)
    return m.eval(), m.clip_model, _clip_batches(cfg)


def _clip_ff():
    from test_clipff_gpu import _model
    from oracle import clip_oracle as O
    cfg = O.tiny_config(embed_dim=128, transformer_width=128, transformer_heads=2)
    m, _ = _model(cfg, dict(d_model=128, num_heads=2, d_ff=256, num_layers=2, d_kv=64), seed=5)
    m.embed_fp16 = False
    return m.eval(), m, _clip_batches(cfg)


def _blip_ff():
    from uniir_amd import blip_model as bm
    m = bm.BLIPFeatureFusion(med_config=MED, vit_config=VIT, embed_dim=128, queue_size=16, momentum=0.9,
                             config=types.SimpleNamespace(tokenizer_max_length=20), seed=4).cuda().eval()
    m.embed_fp16 = False
    g = torch.Generator().manual_seed(7)
    ids = torch.randint(3, MED["vocab_size"], (4, 20), generator=g)
    ids[:, 0] = 1
    mask = (torch.arange(20).unsqueeze(0) < torch.tensor([1, 7, 20, 12]).unsqueeze(1)).long()
    ids, img = ids * mask, torch.randn(4, 3, 32, 32, generator=g)
    return m, m, lambda: [{"txt_batched": types.SimpleNamespace(input_ids=ids[lo:hi].cuda(), attention_mask=mask[lo:hi].cuda()),
                           "image_batched": img[lo:hi].clone(), "did_list": list(range(lo, hi))} for lo, hi in CUTS]


@pytest.mark.parametrize("build", [_clip_sf, _blip_ff, _clip_ff], ids=["clip_sf", "blip_ff", "clip_ff"])
def test_use_fp16_false_is_the_fp32_forward_exactly_when_the_module_opted_in(build):
    E = _embedder()
    model, switch, loader = build()          # switch: the module whose precision the encode path follows

    def extract(use_fp16=False):
        emb, ids = E.generate_embeds_and_ids_for_dataset_with_gather(model, loader(), "cuda:0", use_fp16=use_fp16)
        assert emb.dtype == np.float16 and ids == list(range(4)) and emb.shape[0] == 4
        return torch.from_numpy(emb)

    switch.embed_fp32 = False
    today = extract()                         # bf16, whatever the configuration says
    assert switch.precision == "bf16"
    switch.embed_fp32 = True
    switch.precision = "fp32"                 # by hand (a BLIP or CLIP_FF module knows the value once it has opted in)
    by_hand = extract()
    assert switch.precision == "fp32"         # a value set by hand stays
    switch.precision = "bf16"
    assert not torch.equal(by_hand, today)
    got = extract()
    assert switch.precision == "bf16"         # back afterwards
    assert torch.equal(got, by_hand)
    switch.embed_fp32 = False
    assert torch.equal(extract(), today)      # and without the attribute: today's bits
