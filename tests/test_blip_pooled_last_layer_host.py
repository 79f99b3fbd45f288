"""CPU: the host switch of BLIP's pooled last BERT layer -- BLIPFeatureFusion.pool_last_layer, off by default, switched on at
construction by UNIIR_BLIP_POOL_LAST_LAYER=1 (as UNIIR_POOL_LAST_BLOCK_LONG switches CLIP.pool_last_block_long), inherited by
BLIPScoreFusion -- and the path log it reports to."""
import types

import pytest

MED = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=1, vocab_size=64, max_position_embeddings=32)
VIT = dict(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2)


@pytest.mark.parametrize("score_fusion", [False, True])
def test_attribute_and_environment_variable(monkeypatch, score_fusion):
    from uniir_amd.blip_model import BLIPFeatureFusion, BLIPScoreFusion
    cls = BLIPScoreFusion if score_fusion else BLIPFeatureFusion

    def make():
        return cls(med_config=MED, vit_config=VIT, embed_dim=128, queue_size=8, config=types.SimpleNamespace(tokenizer_max_length=20))

    monkeypatch.delenv("UNIIR_BLIP_POOL_LAST_LAYER", raising=False)
    m = make()
    assert m.pool_last_layer is False and m.path_log == []
    for env, want in (("1", True), ("0", False), ("", False)):
        monkeypatch.setenv("UNIIR_BLIP_POOL_LAST_LAYER", env)
        assert make().pool_last_layer is want, env
    m.path_log.extend(str(i) for i in range(100))
    assert m._path_log() is m.path_log and len(m.path_log) == 63 and m.path_log[-1] == "99"          # the newest lines are kept
