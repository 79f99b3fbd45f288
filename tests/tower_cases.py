"""The case table of tests/test_tower_stages_gpu.py and tests/test_tower_ref.py, with the builders of weights, inputs and the
uniir_clip_tower description.

Not a test module and free of any GPU call.  The shapes are the smallest that still reach each composition path of csrc/tower.hip;
tests/test_tower_ref.py asserts on the host that every case reaches the path it names.
"""
import ctypes as C

import torch

import tower_ref as TR
from tower_ref import Spec

BF16 = torch.bfloat16
LN_BWD_SIDE_DEFAULT = 1           # what uniir_amd.clip_model passes unless UNIIR_LN_BWD_SIDE=0

# EOT positions of T1: the shortest caption a tokenizer emits (SOT, EOT), one token more, a middle one, and the two that fill the context
T1_EOT = (1, 2, 30, 75, 76)
# T2, packed: mixed lengths, 2 and 77 among them (703 live rows of 2310)
T2_EOT = tuple([1, 76] + [(7 * m) % 40 + 3 for m in range(28)])

V1 = dict(is_text=False, W=128, L=2, T=17, E=64, M=3, res=64, patch=16, kpad=768)
V2 = dict(is_text=False, W=256, L=3, T=197, E=136, M=11, res=224, patch=16, kpad=768)
V3 = dict(is_text=False, W=128, L=2, T=577, E=64, M=2, res=384, patch=16, kpad=768)
T1 = dict(is_text=True, W=64, L=2, T=77, E=64, M=5, vocab=512)
T2 = dict(is_text=True, W=256, L=2, T=77, E=64, M=30, vocab=512)


def _lens(eot):
    return tuple(e + 1 for e in eot)


CASES = {}
for _pool in (0, 1):
    CASES[f"V1-pool{_pool}"] = Spec(f"V1-pool{_pool}", pool=_pool, **V1)
    CASES[f"V2-pool{_pool}"] = Spec(f"V2-pool{_pool}", pool=_pool, **V2)
    CASES[f"T1-dense-pool{_pool}"] = Spec(f"T1-dense-pool{_pool}", pool=_pool, **T1)
    CASES[f"T1-packed-pool{_pool}"] = Spec(f"T1-packed-pool{_pool}", pool=_pool, lens=_lens(T1_EOT), **T1)
    CASES[f"T2-dense-pool{_pool}"] = Spec(f"T2-dense-pool{_pool}", pool=_pool, **T2)
    CASES[f"T2-packed-pool{_pool}"] = Spec(f"T2-packed-pool{_pool}", pool=_pool, lens=_lens(T2_EOT), **T2)
for _pool in (0, 1, 2):
    CASES[f"V3-pool{_pool}"] = Spec(f"V3-pool{_pool}", pool=_pool, **V3)


def eot_positions(sp):
    return T1_EOT if sp.M == 5 else T2_EOT


# --------------------------------------------------------------------------------------------------------------------------- data
def make_weights(sp, seed=0, device="cpu", exact=False):
    """fp32 masters under their parameter names and the bf16 shadows under <name>16.  exact: float64 masters, bf16-representable so
    that both the composition and the oracle see the same numbers, and the "shadows" are the masters themselves.  Every LayerNorm
    and every bias is well away from its identity value: a dropped or doubled one moves the result."""
    g = torch.Generator().manual_seed(1000 + seed)
    W, L, E = sp.W, sp.L, sp.E
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g) * std          # noqa: E731
    wt = {}
    for i in range(L):
        b = f"b{i}."
        wt[b + "ln1_w"], wt[b + "ln1_b"] = 1.0 + rn(W, std=0.1), rn(W, std=0.1)
        wt[b + "ln2_w"], wt[b + "ln2_b"] = 1.0 + rn(W, std=0.1), rn(W, std=0.1)
        wt[b + "wqkv"], wt[b + "bqkv"] = rn(3 * W, W, std=W ** -0.5), rn(3 * W, std=0.1)
        wt[b + "wo"], wt[b + "bo"] = rn(W, W, std=W ** -0.5), rn(W, std=0.1)
        wt[b + "wfc"], wt[b + "bfc"] = rn(4 * W, W, std=(2 * W) ** -0.5), rn(4 * W, std=0.1)
        wt[b + "wproj"], wt[b + "bproj"] = rn(W, 4 * W, std=(4 * W) ** -0.5), rn(W, std=0.1)
    if sp.is_text:
        wt["tok"], wt["pos"] = rn(sp.vocab, W, std=0.5), rn(sp.T, W, std=0.5)
    else:
        k = 3 * sp.patch * sp.patch
        conv = torch.zeros(W, sp.kpad)
        conv[:, :k] = rn(W, k, std=k ** -0.5)
        wt["conv"], wt["cls"], wt["pos"] = conv, rn(W, std=0.5), rn(sp.T, W, std=0.5)
        wt["ln_pre_w"], wt["ln_pre_b"] = 1.0 + rn(W, std=0.1), rn(W, std=0.1)
    wt["ln_post_w"], wt["ln_post_b"] = 1.0 + rn(W, std=0.1), rn(W, std=0.1)
    wt["proj"] = rn(W, E, std=W ** -0.5)
    out = {}
    for k, v in wt.items():
        v = v.to(BF16).double() if exact else v
        out[k] = v.to(device)
        if v.dim() == 2 and k not in ("tok", "pos"):
            out[k + "16"] = (v if exact else v.to(BF16)).to(device)
    return out


def make_input(sp, seed=0, device="cpu", exact=False):
    g = torch.Generator().manual_seed(2000 + seed)
    if not sp.is_text:
        img = torch.randn(sp.M, 3, sp.res, sp.res, generator=g)
        return (img.to(BF16).double() if exact else img).to(device)
    sot, eot = sp.vocab - 2, sp.vocab - 1
    txt = torch.zeros(sp.M, sp.T, dtype=torch.int32)          # id 0 behind every EOT
    for m, e in enumerate(eot_positions(sp)):
        txt[m, 0] = sot
        if e > 1:
            txt[m, 1:e] = torch.randint(1, sot, (e - 1,), generator=g, dtype=torch.int32)
        if e > 3:
            txt[m, 2] = txt[m, 1]                             # a repeated id inside one caption
        txt[m, e] = eot
    m = next(m for m, e in enumerate(eot_positions(sp)) if 4 < e < sp.T - 2)
    txt[m, 4] = 0                                             # id 0 as a live token
    return txt.to(device)


def make_demb(sp, seed=0, device="cpu", exact=False):
    g = torch.Generator().manual_seed(3000 + seed)
    d = torch.randn(sp.M, sp.E, generator=g)
    return (d.to(BF16).double() if exact else d).to(device)


def param_shape(sp, name):
    W = sp.W
    base = name.split(".")[-1]
    shapes = dict(ln1_w=(W,), ln1_b=(W,), ln2_w=(W,), ln2_b=(W,), wqkv=(3 * W, W), bqkv=(3 * W,), wo=(W, W), bo=(W,), wfc=(4 * W, W),
                  bfc=(4 * W,), wproj=(W, 4 * W), bproj=(W,), conv=(W, 3 * sp.patch * sp.patch), cls=(W,), pos=(sp.T, W), ln_pre_w=(W,),
                  ln_pre_b=(W,), tok=(sp.vocab, W), ln_post_w=(W,), ln_post_b=(W,), proj=(W, sp.E))
    return shapes[base]


def make_grad_priors(sp, seed=0, device="cpu", exact=False):
    """non-zero starting contents of every gradient buffer (the contract is +=)"""
    g = torch.Generator().manual_seed(4000 + seed)
    out = {}
    for name in sp.params():
        v = torch.randn(*param_shape(sp, name), generator=g) * 0.01
        out["g0." + name] = (v.double() if exact else v).to(device)
    return out


def trace_inputs(sp, seed=0, device="cpu", exact=False):
    tr = {"input": make_input(sp, seed, device, exact), "demb": make_demb(sp, seed, device, exact)}
    tr.update(make_grad_priors(sp, seed, device, exact))
    return tr


# ------------------------------------------------------------------------------------------------------------------------- oracle
def oracle_config(sp):
    return dict(embed_dim=sp.E, image_resolution=sp.res, vision_layers=sp.L, vision_width=sp.W, vision_patch_size=sp.patch,
                context_length=sp.T, vocab_size=sp.vocab, transformer_width=sp.W, transformer_heads=sp.H, transformer_layers=sp.L)


ORACLE_BLOCK = dict(ln1_w="ln_1.weight", ln1_b="ln_1.bias", ln2_w="ln_2.weight", ln2_b="ln_2.bias", wqkv="attn.in_proj_weight",
                    bqkv="attn.in_proj_bias", wo="attn.out_proj.weight", bo="attn.out_proj.bias", wfc="mlp.c_fc.weight",
                    bfc="mlp.c_fc.bias", wproj="mlp.c_proj.weight", bproj="mlp.c_proj.bias")
ORACLE_VISION = dict(cls="visual.class_embedding", pos="visual.positional_embedding", ln_pre_w="visual.ln_pre.weight",
                     ln_pre_b="visual.ln_pre.bias", ln_post_w="visual.ln_post.weight", ln_post_b="visual.ln_post.bias", proj="visual.proj")
ORACLE_TEXT = dict(tok="token_embedding.weight", pos="positional_embedding", ln_post_w="ln_final.weight", ln_post_b="ln_final.bias",
                   proj="text_projection")


def oracle_state(sp, wt):
    """the oracle's state dict (checkpoint names) of a tower's weights -> (sd, {our parameter name: its key}).  conv: the oracle holds
    conv1.weight [W][3][P][P]; ours is that flattened to [W][3 P P] (zero padded to kpad for the GEMM)"""
    pre = "transformer" if sp.is_text else "visual.transformer"
    sd, names = {}, {}
    for i in range(sp.L):
        for ours, theirs in ORACLE_BLOCK.items():
            names[f"b{i}.{ours}"] = f"{pre}.resblocks.{i}.{theirs}"
    names.update(ORACLE_TEXT if sp.is_text else ORACLE_VISION)
    for ours, key in names.items():
        sd[key] = wt[ours].clone().requires_grad_(True)
    if not sp.is_text:
        k = 3 * sp.patch * sp.patch
        names["conv"] = "visual.conv1.weight"
        sd["visual.conv1.weight"] = wt["conv"][:, :k].reshape(sp.W, 3, sp.patch, sp.patch).clone().requires_grad_(True)
    return sd, names


# ------------------------------------------------------------------------------------------------------- the library's description
def describe(sp, ptr, ln_bwd_side=LN_BWD_SIDE_DEFAULT, stash_act=1, recompute=0, splitk=(0, 0)):
    """uniir_clip_tower of a case.  ptr(name) -> address of a weight (<param>, <param>16) or gradient (g.<param>) buffer; the CPU
    tests pass a constant (the layout and workspace queries never touch device memory).  -> (tower, keep-alive)"""
    from uniir_amd import _lib
    blocks = (_lib.ClipBlock * sp.L)()
    for i, b in enumerate(blocks):
        for n in TR.BLOCK_PARAMS:
            if n.startswith("w"):
                setattr(b, n + "16", ptr(f"b{i}.{n}16"))
            else:
                setattr(b, n, ptr(f"b{i}.{n}"))
            setattr(b, "g_" + n, ptr(f"g.b{i}.{n}"))
    t = _lib.ClipTower()
    t.is_text, t.layers, t.width, t.heads, t.tokens, t.embed_dim = int(sp.is_text), sp.L, sp.W, sp.H, sp.T, sp.E
    t.resolution, t.patch, t.kpad, t.vocab = sp.res, sp.patch, sp.kpad, sp.vocab
    t.blocks = C.cast(blocks, C.POINTER(_lib.ClipBlock))
    t.pos_emb, t.ln_post_w, t.ln_post_b, t.proj16 = ptr("pos"), ptr("ln_post_w"), ptr("ln_post_b"), ptr("proj16")
    t.g_pos, t.g_ln_post_w, t.g_ln_post_b, t.g_proj = ptr("g.pos"), ptr("g.ln_post_w"), ptr("g.ln_post_b"), ptr("g.proj")
    if sp.is_text:
        t.token_emb, t.g_token = ptr("tok"), ptr("g.tok")
    else:
        t.conv16, t.class_emb, t.ln_pre_w, t.ln_pre_b = ptr("conv16"), ptr("cls"), ptr("ln_pre_w"), ptr("ln_pre_b")
        t.g_conv, t.g_class, t.g_ln_pre_w, t.g_ln_pre_b = ptr("g.conv"), ptr("g.cls"), ptr("g.ln_pre_w"), ptr("g.ln_pre_b")
    t.splitk_ws, t.splitk_ws_bytes = splitk
    t.ln_bwd_side, t.stash_act, t.dtype16, t.pool_last_block, t.recompute = ln_bwd_side, stash_act, 0, sp.pool, recompute
    return t, blocks


# (region, bytes) of a layout, from the shapes include/uniir_hip.h documents; i: layer sets
def regions(sp, lay):
    """[(name, offset, bytes)] of every region a uniir_clip_tower_layout_t has (absent ones left out), layer sets expanded"""
    R, W, M, H, T, E, G = int(lay.rows), sp.W, sp.M, sp.H, sp.T, sp.E, sp.G
    flat = dict(eot=M * 4, pooled_rows=M * W * 4, pooled=M * W * 2, patches=M * G * sp.kpad * 2, po=M * G * W * 2, x0=R * W * 4,
                x_last=R * W * 4, pl_q=M * W * 2, pl_h1=M * W * 2, pl_x=M * W * 4, pl_ao=M * W * 2, pl_lse=M * H * 4, pl_x2=M * W * 4,
                pl_h2=M * W * 2, pl_f=M * 4 * W * 2, pl_g=M * 4 * W * 2, g=R * 4 * W * 2, df=R * 4 * W * 2, dh=R * W * 2, dx=R * W * 4,
                dx2=R * W * 4, dxb=R * W * 2, dqkv=R * 3 * W * 2, demb16=M * E * 2, dpooled=M * W * 2, drows=M * W * 4,
                pl_dxb=M * W * 2, pl_df=M * 4 * W * 2, pl_dh=M * W * 2, pl_dx2=M * W * 4, pl_dqkv=M * 3 * W * 2, pl_dhq=M * W * 2,
                dx0=R * W * 4, dpo=M * G * W * 2, dconv=W * sp.kpad * 4)
    layer = dict(o_x=R * W * 4, o_qkv=R * 3 * W * 2, o_ao=R * W * 2, o_lse=M * H * T * 4, o_x2=R * W * 4, o_f=R * 4 * W * 2,
                 o_g=R * 4 * W * 2, o_h1=R * W * 2, o_h2=R * W * 2)
    out = [(n, getattr(lay, n), b) for n, b in flat.items() if getattr(lay, n) >= 0]
    sets = sp.L if lay.lay_stride else 1
    for i in range(sets):
        out += [(f"{n}[{i}]", lay.lay0 + i * lay.lay_stride + getattr(lay, n), b) for n, b in layer.items() if getattr(lay, n) >= 0]
    if lay.xs0 >= 0:
        out += [(f"xs[{i}]", lay.xs0 + i * lay.xs_stride, R * W * 4) for i in range(sp.L)]
    return out
