"""The ViT-L/14@336px entry of the CLIP_FF model table (no GPU): the constructor takes the name and builds the T5 stack ViT-L/14 gets."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))


def test_the_table_gives_vit_l14_336_the_stack_of_vit_l14():
    from models.uniir_clip.clip_featurefusion import clip_ff
    assert clip_ff._T5_DMODEL["ViT-L/14@336px"] == clip_ff._T5_DMODEL["ViT-L/14"] == 768


def test_the_constructor_builds_the_336_pixel_model_on_the_host():
    from PIL import Image
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    m = CLIPFeatureFusion("ViT-L/14@336px", device="cpu")
    assert m.clip_model.cfg["image_resolution"] == 336
    assert tuple(m.t5_layers.get_parameter("block.0.layer.0.SelfAttention.q.weight").shape) == (768, 768)
    assert tuple(m.t5_layers.get_parameter("block.0.layer.0.SelfAttention.relative_attention_bias.weight").shape) == (32, 12)
    assert tuple(m.get_img_preprocess_fn()(Image.new("RGB", (500, 400))).shape) == (3, 336, 336)
    assert not hasattr(m.clip_model, "text_projection")


def test_other_names_are_still_refused():
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    with pytest.raises(NotImplementedError):
        CLIPFeatureFusion("ViT-B/16", device="cpu")


def test_the_stack_takes_the_streaming_entry_points_above_512_tokens_only():
    from uniir_amd import clipff_model as FM
    assert FM._rel_entry("fwd", 512) == "uniir_attention_rel_fwd" and FM._rel_entry("bwd", 334) == "uniir_attention_rel_bwd"
    assert FM._rel_entry("fwd", 513) == "uniir_attention_rel_fwd_long" and FM._rel_entry("bwd", 654) == "uniir_attention_rel_bwd_long"
    assert len(FM.rel_bucket_table(654)) == 2 * 654 - 1
