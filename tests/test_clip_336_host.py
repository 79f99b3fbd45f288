"""The ViT-L/14@336px entry of the CLIP model table (no GPU)."""
import pytest


def test_vit_l14_336_is_vit_l14_at_336_pixels():
    from uniir_amd.clip_model import CLIP_CONFIGS
    big, base = dict(CLIP_CONFIGS["ViT-L/14@336px"]), dict(CLIP_CONFIGS["ViT-L/14"])
    assert big.pop("image_resolution") == 336
    assert base.pop("image_resolution") == 224
    assert big == base
    assert (336 // big["vision_patch_size"]) ** 2 + 1 == 577


def test_load_lists_the_new_name_among_the_available_models():
    from uniir_amd import clip_front
    with pytest.raises(RuntimeError) as e:
        clip_front.load("nope")
    assert "ViT-L/14@336px" in str(e.value)
