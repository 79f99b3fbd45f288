"""CPU tests of uniir_amd/flat_store.py: the flat layout every model keeps its parameters in.  Checkpoints, optimizer state, the
bucketed gradient all-reduce and the C tower's raw pointers all depend on it, so the layout is restated here independently."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "uniir_amd", "src")
for p in (ROOT, SRC):
    if p not in sys.path:
        sys.path.insert(0, p)

BLOCK_WEIGHTS = ("attn.in_proj_weight", "attn.out_proj.weight", "mlp.c_fc.weight", "mlp.c_proj.weight")


def _granules(numel):
    """elements a tensor occupies: whole 64-element (256-B) granules"""
    return -(-numel // 64) * 64


def test_clip_store_layout_ranges_and_adoption():
    from oracle import clip_oracle as O
    from uniir_amd.clip_model import CLIP
    from uniir_amd.flat_store import ALIGN, FlatStore
    cfg = O.tiny_config()
    clip = CLIP(cfg, seed=3)
    named = list(clip.named_parameters())
    before = {n: p.detach().clone() for n, p in named}
    st = FlatStore.adopt(clip._flat_order(), "cpu")

    # order: gains / biases / logit_scale first, then the weight-decay tensors, each in named_parameters() order
    no_decay = [n for n, p in named if p.ndim < 2 or any(k in n for k in ("bn", "ln", "bias", "logit_scale"))]
    decay = [n for n, _ in named if n not in no_decay]
    assert list(st.off) == no_decay + decay and no_decay and decay
    assert all(o % ALIGN == 0 for o in st.off.values())
    size = {n: _granules(p.numel()) for n, p in named}
    split = sum(size[n] for n in no_decay)
    total = split + sum(size[n] for n in decay)
    assert st.total == total and st.off[decay[0]] == split
    assert st.ranges(clip.adamw_group) == [(0, split, 0), (split, total, 1)]

    # a residual block's four weight matrices are one adjacent range: one bucket of the overlapped all-reduce
    clip._flat = st
    for prefix, layers in (("visual.transformer", cfg["vision_layers"]), ("transformer", cfg["transformer_layers"])):
        for i in range(layers):
            names = [f"{prefix}.resblocks.{i}.{w}" for w in BLOCK_WEIGHTS]
            lo, hi = clip.layer_grad_range(prefix, i)
            assert (lo, hi) == st.span(names) and lo == min(st.off[n] for n in names) and hi - lo == sum(size[n] for n in names)
    with pytest.raises(RuntimeError):
        st.span(["transformer.resblocks.0.attn.in_proj_weight", "transformer.resblocks.1.attn.in_proj_weight"])

    # adopting: every parameter is a view of the master buffer (values kept), its .grad a view of the gradient buffer
    for n, p in clip.named_parameters():
        assert p.data_ptr() == st.p32.data_ptr() + 4 * st.off[n] and torch.equal(p.detach(), before[n])
        assert p.grad.data_ptr() == st.g32.data_ptr() + 4 * st.off[n] and p.grad.shape == p.shape
    assert st.holds(clip.named_parameters())
    st.p("logit_scale").fill_(2.5)
    assert float(clip.logit_scale.detach()) == 2.5 and st["p32"] is st.p32 and st["g32"] is st.g32 and st["off"] is st.off
    assert st.ptr(st.w16_buf, "visual.proj") == st.w16_buf.data_ptr() + 2 * st.off["visual.proj"]

    clip.visual.proj.grad = torch.ones_like(clip.visual.proj)          # replaced by torch: zero_grad points it back
    st.g32.fill_(1.0)
    clip.zero_grad()
    assert clip.visual.proj.grad.data_ptr() == st.ptr(st.g32, "visual.proj") and not st.g32.any()
    clip.visual.proj.data = clip.visual.proj.data.clone()                # no longer a view: the store must be rebuilt
    assert not st.holds(clip.named_parameters())


def test_blip_sf_stores_skip_the_frozen_cross_attention():
    from uniir_amd.blip_model import BLIPScoreFusion
    from uniir_amd.flat_store import FlatStore
    med = dict(hidden_size=64, intermediate_size=128, max_position_embeddings=16, num_attention_heads=1, num_hidden_layers=2,
               vocab_size=100)
    vit = dict(patch_size=16, embed_dim=64, depth=2, num_heads=1, drop_path_rate=0.0, img_size=32)
    m = BLIPScoreFusion(med_config=med, vit_config=vit, embed_dim=32, queue_size=8)
    online = FlatStore.adopt(m._online_params(), "cpu", frozen=m._frozen)
    mom = FlatStore.adopt(m._momentum_params(), "cpu", with_grad=False)
    names = list(online.off)
    first_frozen = min(online.off[n] for n in m._frozen)
    assert m._frozen and names[-1] == "temp" and all(names.index(n) > names.index("text_proj.bias") for n in m._frozen)
    assert online.ranges(m.adamw_group) == [(0, first_frozen, 1), (online.off["temp"], online.total, 1)]
    for n, p in m._online_params():
        assert (p.grad is None) == (n in m._frozen)
        assert n in m._frozen or p.grad.data_ptr() == online.ptr(online.g32, n)
    # the momentum store: the online layout without temp, no gradient buffer
    assert mom.g32 is None and list(mom.off) == names[:-1] and all(mom.off[n] == online.off[n] for n in mom.off)
    assert mom.holds(m._momentum_params()) and online.holds(m._online_params())
    for n, pm in m._momentum_params():
        assert torch.equal(pm.detach(), m.get_parameter(n).detach())


def test_native_adamw_state_dict_keys():
    """optimizer state saved before the stores were unified keeps loading: the same keys and shapes"""
    from oracle import clip_oracle as O
    from uniir_amd.clip_model import CLIP
    from uniir_amd.trainer import NativeAdamW
    opt = NativeAdamW(CLIP(O.tiny_config(), seed=3), lr=1e-3)
    sd = opt.state_dict()
    assert set(sd) == {"opt_step", "exp_avg", "exp_avg_sq", "extra", "param_groups"} and sd["exp_avg"] is None
    assert [g["weight_decay"] for g in sd["param_groups"]] == [0.0, 0.2]
    m, v = torch.randn(100), torch.randn(100)
    opt.load_state_dict(dict(sd, opt_step=7, exp_avg=m, exp_avg_sq=v))
    again = opt.state_dict()
    assert again["opt_step"] == 7 and again["exp_avg"] is m and again["exp_avg_sq"] is v and again["extra"] == []


# ---- NativeAdamW and the store's one "a kernel wrote the masters" event --------------------------------------------------------------
def _recorded_step(monkeypatch, guarded):
    """a BLIP-shaped pair of stores (the online one is stepped, the momentum one is not) plus an extra store without padded tensors
    (CLIP_FF's T5 stack), on the CPU with ops.call recorded -> (online, momentum, extra, the calls of one step as (name, store tag))"""
    from types import SimpleNamespace
    from uniir_amd import ops
    from uniir_amd.blip_model import CONV, BLIPScoreFusion
    from uniir_amd.flat_store import FlatStore, patch_kpad
    from uniir_amd.trainer import NativeAdamW
    med = dict(hidden_size=64, intermediate_size=128, max_position_embeddings=16, num_attention_heads=1, num_hidden_layers=2,
               vocab_size=100)
    vit = dict(patch_size=16, embed_dim=64, depth=2, num_heads=1, drop_path_rate=0.0, img_size=32)
    m = BLIPScoreFusion(med_config=med, vit_config=vit, embed_dim=32, queue_size=8)
    online = FlatStore.adopt(m._online_params(), "cpu", frozen=m._frozen, unversioned=("temp",))
    mom = FlatStore.adopt(m._momentum_params(), "cpu", with_grad=False)
    for st in (online, mom):
        st.add_padded("visual_encoder." + CONV, 64, 768, patch_kpad(16))
    t5_params = [torch.nn.Parameter(torch.randn(8, 8)), torch.nn.Parameter(torch.randn(8))]
    extra = FlatStore.adopt([("a", t5_params[0]), ("b", t5_params[1])], "cpu")
    tag = {online.p32.data_ptr(): "online", mom.p32.data_ptr(): "momentum", extra.p32.data_ptr(): "extra"}
    calls = []

    def call(name, *a):
        src = a[0]
        base = src.untyped_storage().data_ptr()
        calls.append((name, tag[base]))

    monkeypatch.setattr(ops, "call", call)
    model = SimpleNamespace(_ensure_flat=lambda: online, optimizer_groups=m.optimizer_groups, adamw_group=m.adamw_group)
    group = SimpleNamespace(params=t5_params, store=lambda: extra, weight_decay=0.2, lr=1e-3)
    opt = NativeAdamW(model, lr=1e-3, allreduce=False, extra=[group], max_grad_norm=1.0 if guarded else None, skip_nonfinite=False)
    assert (opt.guard is not None) == guarded
    if guarded:          # the guard's own launches need the device: stood in for, in their place in the sequence
        opt.guard = SimpleNamespace(ctl=None, resolve=lambda: False, publish=lambda: calls.append(("publish", None)),
                                    measure=lambda ranges, scale: calls.append(("measure", None)))
    for st in (online, mom, extra):
        st.half_stale = False          # as if fp16 copies existed and were fresh
    opt.step()
    return online, mom, extra, calls


@pytest.mark.parametrize("guarded", [False, True])
def test_native_adamw_tells_every_store_it_stepped_exactly_once(monkeypatch, guarded):
    """per store: the AdamW launches, then FlatStore.kernel_wrote() -- one pad launch for the online store's one padded tensor, none
    for the momentum store (the optimizer does not step it) and none for a store without padded tensors; fp16 goes stale where stepped"""
    online, mom, extra, calls = _recorded_step(monkeypatch, guarded)
    step = "uniir_adamw_step_guarded" if guarded else "uniir_adamw_step"
    body = [c for c in calls if c[0] not in ("measure", "publish")]
    launches = [c for c in body if c[1] == "online" and c[0] == step]
    assert len(launches) == 2          # trainable | frozen cross-attention (not stepped) | temp: two ranges
    assert body == launches + [("uniir_cast_pad_rows", "online"), (step, "extra")]
    assert not any(c[1] == "momentum" for c in calls)
    if guarded:
        assert calls[0] == ("measure", None) and calls[-1] == ("publish", None) and len(calls) == len(body) + 2
    assert online.half_stale is True and extra.half_stale is True and mom.half_stale is False
    assert online.half_bytes() == 0 and extra.half_bytes() == 0          # and nothing fp16 was allocated by the step
