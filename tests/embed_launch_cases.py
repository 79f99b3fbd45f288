"""The launch sequences of the embedding forwards as data (tests/test_embed_launches_host.py and
tests/golden/make_golden_embed_launches.py), next to tests/bert_launch_cases.py, whose recorder, digest and entry format these cases
use: the fp32 forwards of CLIP, CLIP_FF (towers without pooling, T5 stack), the BLIP ViT, the MED BERT and BLIP_SF, and the 16-bit
forward-only passes (save False) of the BLIP ViT, the CLIP_FF towers, the T5 stack and BLIP_SF in bf16 and fp16.  (bert_forward in
16 bits is pinned by g19.)  CPU FlatStores, every ops function a case meets replaced by a recorder: no GPU, no library.

Unlike g19's, an entry here holds the call as the op's own signature binds it, defaults filled in: f(x) and f(x, eps=1e-5) are one
launch and one entry.  Width 128, 2 heads, 2 layers everywhere, so that the carry between layers shows."""
import inspect
import json
import re
import types

import torch

import bert_launch_cases as K
from bert_launch_cases import digest, first_difference  # noqa: F401  (the test and the generator take them from here, too)

W, HEADS, LAYERS = 128, 2, 2
T5_M, T5_T, T5_DFF = 2, 6, 256
VIT = dict(img_size=32, patch_size=16, embed_dim=W, depth=LAYERS, num_heads=HEADS, drop_path_rate=0.0)
MED = dict(hidden_size=W, intermediate_size=K.I, num_attention_heads=HEADS, num_hidden_layers=LAYERS, vocab_size=64,
           max_position_embeddings=16)
DT = {"bf16": torch.bfloat16, "fp16": torch.float16}

FP32 = ("clip-image", "clip-text", "clipff-vision", "clipff-text", "t5", "vit", "bert-cross-pool", "bert-cross", "bert-text", "sf")
HALF = ("vit", "clipff-vision", "clipff-text", "t5", "sf")
NAMES = [f"fp32-{n}" for n in FP32] + [f"{d}-{n}" for d in DT for n in HALF]
CASES = NAMES          # a case is its name

# The fp32 pre-LN block body is one function for the CLIP towers and the BLIP ViT (fp32_forward.tower_fwd_f32), and it puts every
# LayerNorm output into a fresh buffer, as the BLIP ViT always did; the CLIP towers used to send ln_1 and ln_2 of a block through one
# buffer h.  So in these cases, and in no other, WHICH temporary holds a LayerNorm output differs from the recorded parent: their
# digests are taken with the #n of non-store buffers blanked, and still cover the op, every shape, stride and offset, every operand
# that is a view of the store and every scalar.
LOOSE = ("fp32-clip-image", "fp32-clip-text", "fp32-clipff-vision", "fp32-clipff-text")
FULL = ("fp32-sf",)          # held in the fixture entry by entry


class BoundRecorder(K.Recorder):
    def wrap(self, name, result):
        sig = inspect.signature(self.real[name])

        def f(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            args = dict(bound.arguments)
            entry = [name, self.enc(args.pop("args", ())), {k: self.enc(v) for k, v in sorted(args.items())}, None]
            self.entries.append(entry)
            out = result(*a, **kw)
            entry[3] = self.enc(out)
            return out
        return f


def _fakes():
    """bert_launch_cases' stand-ins plus those of the ops only the towers and the T5 stack use"""
    fakes = K._fakes()

    def attention_fwd(qkv, batch, seq, heads, causal=False, *, out=None, lse=None):
        return (out if out is not None else torch.empty(batch * seq, heads * 64, dtype=qkv.dtype),
                lse if lse is not None else torch.empty(batch, heads, seq))

    def attention_rel_fwd_f16(qkv, rel_emb, table, batch, seq, heads, scale=1.0):
        return torch.empty(batch * seq, heads * 64, dtype=torch.float16), torch.empty(batch, heads, seq)

    def rmsnorm_fwd(x, gamma, eps, *, out_bf16=None, out_f32=None, rows=None, width=None, x_stride=None, dtype16=torch.bfloat16):
        if out_bf16 is None and out_f32 is None:
            out_bf16 = torch.empty(rows, width, dtype=dtype16)
        return out_bf16 if out_bf16 is not None else out_f32

    fakes.update(attention_fwd=attention_fwd, attention_fwd_causal_f16=attention_fwd, attention_rel_fwd_f16=attention_rel_fwd_f16,
                 rmsnorm_fwd=rmsnorm_fwd)
    return fakes


def _padded(st, name, width, P, half):
    """what a model does to its store before the forward: the patch weight `name` registered for its padded copies and, for an fp16
    forward, the fp16 copies brought up to date (nothing is launched here, and these calls are no part of a trace)"""
    from uniir_amd import flat_store, ops
    st.add_padded(name, width, 3 * P * P, flat_store.patch_kpad(P))
    if half:
        real, ops.call = ops.call, lambda *a: None
        try:
            st.half_shadow()
        finally:
            ops.call = real
    return st


def _clip(patches16, half):
    """what the CLIP launch sequences read of a CLIP module: its config and its store, which holds the padded patch weights where
    the case reads them (patches16: the 16-bit vision tower)"""
    from oracle import clip_oracle
    from uniir_amd import clip_model, flat_store
    cfg = clip_oracle.tiny_config(embed_dim=W, transformer_width=W, transformer_heads=HEADS)
    st = flat_store.FlatStore([(n, tuple(p.shape)) for n, p in clip_model.CLIP(cfg).named_parameters()], "cpu")
    if patches16:
        _padded(st, clip_model.CONV, cfg["vision_width"], cfg["vision_patch_size"], half)
    model = types.SimpleNamespace(cfg=cfg, _flat=st, kpad=flat_store.patch_kpad(cfg["vision_patch_size"]), recompute_blocks=False)
    image = torch.zeros(2, 3, cfg["image_resolution"], cfg["image_resolution"])
    return model, st, image, torch.zeros(2, cfg["context_length"], dtype=torch.int32)


def _blip_sf():
    from uniir_amd import blip_model as bm, flat_store
    model = bm.BLIPScoreFusion(med_config=MED, vit_config=VIT, embed_dim=W, queue_size=16, momentum=0.9,
                               config=types.SimpleNamespace(tokenizer_max_length=K.L), seed=0).eval()
    return model, flat_store.FlatStore(model._shapes, "cpu")


def _run(prec, what):
    """-> (the store the case runs on, a function that runs it and returns what the forward returned)"""
    from uniir_amd import blip_model as bm, clip_model, clipff_model as fm, flat_store
    f32, dt = prec == "fp32", DT.get(prec)
    ids, key_len = torch.zeros(K.M, K.L, dtype=torch.int32), torch.tensor(K.KEY_LEN, dtype=torch.int32)
    images = torch.zeros(2, 3, VIT["img_size"], VIT["img_size"])
    if what.startswith("clip"):
        model, st, image, text = _clip(what == "clipff-vision" and not f32, prec == "fp16")
        if what == "clip-image":
            return st, lambda: clip_model._encode_fp32(model, "image", image, st.p)
        if what == "clip-text":
            return st, lambda: clip_model._encode_fp32(model, "text", text, st.p)
        if what == "clipff-vision":
            return st, (lambda: fm.vision_tokens_f32(model, image)) if f32 else (lambda: fm.vision_tokens_fwd(model, image, False, dt))
        return st, (lambda: fm.text_tokens_f32(model, text)) if f32 else (lambda: fm.text_tokens_fwd(model, text, False, dt))
    if what == "t5":
        st = flat_store.FlatStore(fm.t5_param_shapes(W, HEADS, 64, T5_DFF, LAYERS), "cpu")
        x = torch.zeros(T5_M * T5_T, W)
        if f32:
            return st, lambda: fm.t5_forward_f32(st, "", x, T5_M, T5_T, HEADS, LAYERS)
        return st, lambda: fm.t5_forward(st, "", x, T5_M, T5_T, HEADS, LAYERS, False, dtype16=dt)
    if what == "vit":
        st = flat_store.FlatStore([("visual_encoder." + n, s) for n, s in bm.vit_param_shapes(VIT, VIT["img_size"])], "cpu")
        if f32:
            return st, lambda: bm.vit_forward_f32(st, "visual_encoder.", VIT, VIT["img_size"], images)
        _padded(st, "visual_encoder." + bm.CONV, W, VIT["patch_size"], prec == "fp16")
        return st, lambda: bm.vit_forward(st, "visual_encoder.", VIT, VIT["img_size"], images, False, dtype16=dt)
    if what.startswith("bert"):
        cross, pool = what != "bert-text", what == "bert-cross-pool"
        cfg = {**bm.MED_DEFAULT, **MED}
        st = flat_store.FlatStore([("text_encoder." + n, s) for n, s in bm.bert_param_shapes(cfg, K.ENC, pooler=cross)], "cpu")
        img = torch.zeros(K.M * K.TI, K.ENC) if cross else None
        return st, lambda: bm.bert_forward_f32(st, "text_encoder.", cfg, ids, key_len, img, K.TI if cross else 0, cross=cross, pool=pool)
    assert what == "sf"
    model, st = _blip_sf()
    images = torch.zeros(K.M, 3, VIT["img_size"], VIT["img_size"])
    ones = torch.ones(K.M, dtype=torch.int64)
    if f32:
        return st, lambda: model._encode_sf_f32(st, ids, key_len, images, ones, ones)
    pack = bm.TextPack.build(key_len, K.L)
    _padded(st, "visual_encoder." + bm.CONV, W, VIT["patch_size"], prec == "fp16")
    return st, lambda: model._encode_sf(st, ids, key_len, images, ones, ones, False, pack, dt)


def trace(name):
    """the entries of one case, then what the forward returned"""
    st, run = _run(*name.split("-", 1))
    with K.recording(st, _fakes(), BoundRecorder) as rec:
        out = run()
        return rec.entries + [["returned", rec.enc(out)]]


def normalised(name, entries):
    """the entries the digests of case `name` are taken of: those of a LOOSE case without the numbers of their non-store buffers"""
    return json.loads(re.sub(r"@#\d+", "@#", json.dumps(entries))) if name in LOOSE else json.loads(json.dumps(entries))
