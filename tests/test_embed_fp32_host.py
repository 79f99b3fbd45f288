"""Host logic of the fp32 embedding forward, no GPU: the embedder's rule (mbeir_embedder._tower_precision: use_fp16 False switches a
module that opted in with embed_fp32 from "bf16" to "fp32" for the extraction and back afterwards; nothing else changes), the
embed_fp32 attribute of the three modules and UNIIR_EMBED_FP32, the precision guards of BLIP_FF / BLIP_SF / CLIP_FF -- train mode, grad
mode, the momentum encoder, unknown values and "fp32" on a module that has not opted in raise before any launch -- and the binding of uniir_attn_f32_rel_fwd."""
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))

MED_TINY = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=1, vocab_size=64,
                max_position_embeddings=32)
VIT_TINY = dict(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, drop_path_rate=0.0)


def _embedder():
    src = os.path.join(ROOT, "uniir_amd", "src")
    for p in (src, os.path.join(src, "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import mbeir_embedder
    return mbeir_embedder


def _stand_ins(kind, embed_fp32, precision="bf16", wrap=False):
    """-> (model, the module whose precision the encode path follows, every module that carries a precision)"""
    ns = types.SimpleNamespace
    if kind == "clip_sf":          # a model around a CLIP module; the CLIP module carries precision and embed_fp32
        clip = ns(precision=precision, embed_fp32=embed_fp32)
        model, main, all_ = ns(clip_model=clip), clip, [clip]
    elif kind == "blip":
        model = ns(precision=precision, embed_fp16=False, embed_fp32=embed_fp32)
        main, all_ = model, [model]
    else:                          # CLIP_FF: the module's own precision decides; the inner CLIP module carries one too
        clip = ns(precision=precision, embed_fp32=embed_fp32)
        model = ns(clip_model=clip, precision=precision, embed_fp16=False, embed_fp32=embed_fp32)
        main, all_ = model, [model, clip]
    return (ns(module=model) if wrap else model), main, all_


@pytest.mark.parametrize("wrap", [False, True], ids=["bare", "module"])
@pytest.mark.parametrize("kind", ["clip_sf", "blip", "clip_ff"])
def test_use_fp16_false_means_fp32_only_for_a_module_that_opted_in_and_the_old_value_comes_back(kind, wrap):
    E = _embedder()
    model, main, all_ = _stand_ins(kind, True, wrap=wrap)
    with E._tower_precision(model, False):
        assert main.precision == "fp32"
    assert all(m.precision == "bf16" for m in all_)
    with pytest.raises(KeyError):          # also when the body raises
        with E._tower_precision(model, False):
            assert main.precision == "fp32"
            raise KeyError("body")
    assert all(m.precision == "bf16" for m in all_)
    # without embed_fp32 nothing changes, whatever use_fp16 says about fp32
    model, main, all_ = _stand_ins(kind, False, wrap=wrap)
    with E._tower_precision(model, False):
        assert all(m.precision == "bf16" for m in all_)
    assert all(m.precision == "bf16" for m in all_)
    # a precision set by hand stays, inside and afterwards
    for by_hand in ("fp16", "fp32"):
        model, main, all_ = _stand_ins(kind, True, precision=by_hand, wrap=wrap)
        for use_fp16 in (False, True):
            with E._tower_precision(model, use_fp16):
                assert all(m.precision == by_hand for m in all_)
            assert all(m.precision == by_hand for m in all_)


@pytest.mark.parametrize("embed_fp32", [False, True])
@pytest.mark.parametrize("kind", ["clip_sf", "blip", "clip_ff"])
def test_use_fp16_true_behaves_as_it_did_with_and_without_embed_fp32(kind, embed_fp32):
    E = _embedder()
    model, main, all_ = _stand_ins(kind, embed_fp32)
    with E._tower_precision(model, True):
        # the CLIP module takes its fp16 forward as always; BLIP and the CLIP_FF module only with embed_fp16, which is off here
        assert [m.precision for m in all_] == {"clip_sf": ["fp16"], "blip": ["bf16"], "clip_ff": ["bf16", "fp16"]}[kind]
    assert all(m.precision == "bf16" for m in all_)
    if kind != "clip_sf":
        main.embed_fp16 = True
        with E._tower_precision(model, True):
            assert main.precision == "fp16"
        assert main.precision == "bf16"
        with E._tower_precision(model, False):          # embed_fp16 says nothing about use_fp16: False
            assert main.precision == ("fp32" if embed_fp32 else "bf16")
        assert main.precision == "bf16"


def test_a_stand_in_without_the_attribute_is_left_alone():
    E = _embedder()
    blip = types.SimpleNamespace(precision="bf16", embed_fp16=True)          # a module from before embed_fp32 existed
    with E._tower_precision(blip, False):
        assert blip.precision == "bf16"


def _blip(cls):
    from uniir_amd import blip_model as bm
    return getattr(bm, cls)(med_config=MED_TINY, vit_config=VIT_TINY, embed_dim=128, queue_size=16, momentum=0.9,
                            config=types.SimpleNamespace(tokenizer_max_length=4), seed=0)


def test_embed_fp32_is_off_by_default_and_the_environment_opts_every_module_in(monkeypatch):
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from oracle import clip_oracle as O
    from uniir_amd import clip_model
    cfg = O.tiny_config(embed_dim=128, transformer_width=128, transformer_heads=2)
    clip_model.CLIP_CONFIGS["tiny-ff"] = cfg
    make = (lambda: clip_model.CLIP(cfg), lambda: _blip("BLIPFeatureFusion"), lambda: _blip("BLIPScoreFusion"),
            lambda: CLIPFeatureFusion("tiny-ff", device="cpu", t5_config=dict(d_model=128, num_heads=2, d_ff=256, num_layers=2)))
    for value, want in ((None, False), ("0", False), ("", False), ("1", True)):
        if value is None:
            monkeypatch.delenv("UNIIR_EMBED_FP32", raising=False)
        else:
            monkeypatch.setenv("UNIIR_EMBED_FP32", value)
        for f in make:
            m = f()
            assert m.embed_fp32 is want and m.precision == "bf16", (value, type(m).__name__)          # opts in; the default stays
    ff = make[3]()
    assert ff.clip_model.embed_fp32 is True          # the inner CLIP module of CLIP_FF follows the same variable


@pytest.mark.parametrize("cls", ["BLIPFeatureFusion", "BLIPScoreFusion"])
def test_blip_precision_guards(cls):
    model = _blip(cls).eval()
    txt = types.SimpleNamespace(input_ids=torch.zeros(2, 4, dtype=torch.int64), attention_mask=torch.ones(2, 4, dtype=torch.int64))
    img = torch.zeros(2, 3, 32, 32)
    model.precision, model.embed_fp32 = "fp32", False
    for grad in (True, False):          # a module that has not opted in does not know the value, as before the fp32 forward existed
        with pytest.raises(RuntimeError, match="unknown precision 'fp32'"), torch.set_grad_enabled(grad):
            model.encode_multimodal_input(txt, img)
    model.embed_fp32 = True
    with pytest.raises(RuntimeError, match="no_grad"):          # grad mode
        model.encode_multimodal_input(txt, img)
    with pytest.raises(RuntimeError, match="online"), torch.no_grad():          # the momentum encoder
        model.encode_multimodal_input(txt, img, use_momentum=True)
    model.train()
    with pytest.raises(RuntimeError, match="eval"), torch.no_grad():          # train mode
        model.encode_multimodal_input(txt, img)
    with pytest.raises(RuntimeError, match="eval"):
        model({"txt_batched": txt, "image_batched": img, "did_list": [0, 1]}, encode_mbeir_batch=True)
    model.eval()
    for bad in ("fp64", "FP32", "float32", None):
        model.precision = bad
        with pytest.raises(RuntimeError, match="unknown precision"), torch.no_grad():
            model.encode_multimodal_input(txt, img)
    model.precision = "fp32"          # past the guards there is no CPU path: the device is asked for, not a fallback taken
    with pytest.raises(RuntimeError, match="MI355X"), torch.no_grad():
        model.encode_multimodal_input(txt, img)


def test_clipff_precision_guards():
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from oracle import clip_oracle as O
    from uniir_amd import clip_model
    clip_model.CLIP_CONFIGS["tiny-ff"] = O.tiny_config(embed_dim=128, transformer_width=128, transformer_heads=2)
    m = CLIPFeatureFusion("tiny-ff", device="cpu", t5_config=dict(d_model=128, num_heads=2, d_ff=256, num_layers=2)).eval()
    txt, img = torch.zeros(2, 77, dtype=torch.int64), torch.zeros(2, 3, 64, 64)
    m.precision, m.embed_fp32 = "fp32", False
    for grad in (True, False):          # a module that has not opted in does not know the value, as before the fp32 forward existed
        with pytest.raises(RuntimeError, match="unknown precision 'fp32'"), torch.set_grad_enabled(grad):
            m.encode_multimodal_input(txt, img)
    m.embed_fp32 = True
    with pytest.raises(RuntimeError, match="no_grad"):          # grad mode
        m.encode_multimodal_input(txt, img)
    m.train()
    with pytest.raises(RuntimeError, match="eval"), torch.no_grad():
        m.encode_multimodal_input(txt, img)
    m.eval()
    for bad in ("fp64", "FP32", "float32", None):
        m.precision = bad
        with pytest.raises(RuntimeError, match="unknown precision"), torch.no_grad():
            m.encode_multimodal_input(txt, img)
    m.precision = "fp32"
    with pytest.raises(RuntimeError, match="MI355X"), torch.no_grad():
        m.encode_multimodal_input(txt, img)


def test_the_binding_knows_the_entry_point():
    from uniir_amd import _lib
    name = "uniir_attn_f32_rel_fwd"
    res, args = _lib.SIGNATURES[name]
    twin = _lib.SIGNATURES["uniir_attn_rel_fwd_f16"][1]
    assert not name.startswith("uniir_attention_") and len(args) == len(twin) - 1          # the fp16 twin minus lse
    lib = _lib.load()
    assert callable(getattr(lib, name)) and lib.uniir_abi_version() >= 7
    # refusals need no device: a refused call launches nothing
    assert lib.uniir_attn_f32_rel_fwd(None, None, None, None, 32, 1.0, 1, 8, 2, None) == -1
    assert lib.uniir_attn_f32_rel_fwd(4096, 8192, 12288, 16384, 65, 1.0, 1, 8, 2, None) == -1
    assert lib.uniir_attn_f32_rel_fwd(4096, 8192, 12288, 16384, 32, 1.0, 1, 1025, 2, None) == -2
    assert lib.uniir_attn_f32_rel_fwd(4096, 8192, 12288, 16384, 32, 1.0, 0, 8, 2, None) == 0
