"""The host side of block recomputation in the per-op towers (uniir_amd/resblocks.py): the boundary the BLIP models derive from the
reference's vit_grad_ckpt / vit_ckpt_layer keys, and the size of one rebuilt block set.  No GPU."""
import types

import pytest


@pytest.mark.parametrize("depth,flag,layer,want", [(24, True, 12, 12), (24, True, 0, 24), (24, False, 12, 24), (12, True, 99, 0),
                                                   (4, True, -1, 4)])
def test_vit_recompute_from_follows_the_reference_rule(depth, flag, layer, want):
    """backbone/vit.py:230 wraps the blocks i >= depth - ckpt_layer when use_grad_checkpointing is set"""
    from uniir_amd.blip_model import vit_recompute_from
    assert vit_recompute_from(depth, flag, layer) == want


MED = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=2, vocab_size=64,
           max_position_embeddings=32)
VIT = dict(img_size=64, patch_size=16, embed_dim=128, depth=4, num_heads=2)


@pytest.mark.parametrize("score_fusion", [False, True])
def test_constructor_keeps_the_boundary(score_fusion):
    from uniir_amd.blip_model import BLIPFeatureFusion, BLIPScoreFusion
    cls = BLIPScoreFusion if score_fusion else BLIPFeatureFusion
    kw = dict(med_config=MED, vit_config=VIT, embed_dim=128, queue_size=16, config=types.SimpleNamespace(tokenizer_max_length=20))
    assert cls(vit_grad_ckpt=True, vit_ckpt_layer=2, **kw).vit_recompute_from == 2
    assert cls(**kw).vit_recompute_from == 4
    assert cls(vit_grad_ckpt=False, vit_ckpt_layer=2, **kw).vit_recompute_from == 4


def test_block_set_bytes_is_the_documented_sum():
    from uniir_amd.resblocks import block_set_bytes
    # 102 rows of width 128, 2 heads: 24 * 128 + 4 * 2 = 3080 bytes per row
    assert block_set_bytes(102, 128, 2) == 314160
    # ViT-L at 256 images of 197 tokens: 50432 rows x (24 * 1024 + 4 * 16 = 24640)
    assert block_set_bytes(50432, 1024, 16) == 1242644480
