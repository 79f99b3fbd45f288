"""MI355X-native CLIP feature-fusion encoder: the CLIP towers WITHOUT pooling
(src/models/uniir_clip/clip_featurefusion/clip_ff.py:35-59 vision: ln_post + proj on all tokens; :148-156 text: ln_final on
all tokens, no EOT pooling / projection), the token concat, the 2-layer T5 encoder stack (transformers T5Stack: RMS norm,
un-scaled attention with bucketed relative position bias, ReLU feed-forward, no biases) and the mean over tokens (:161-192).

All arithmetic is in libuniir_hip.so; this file is the launch sequence + the flat store of the T5 parameters (state-dict
keys `t5_layers.block.{i}.layer.{0,1}...` of transformers).  In train mode the T5 dropout sites (dropout_rate 0.1: stack
input, attention probabilities, attention output, after the ReLU, feed-forward output, after the final norm) are applied
with counter-based masks regenerated in backward (ops.DropSeeds); the CLIP towers have no dropout.

dtype16 = torch.float16 (t5_forward, vision_tokens_fwd, text_tokens_fwd): the eval-mode embedding forward with fp16 16-bit
activations and weights from the stores' fp16 shadows (FlatStore.w16h) -- the same launch sequence, the fp16 twins of the entry
points (uniir_rmsnorm_fwd_f16, uniir_attn_rel_fwd_f16 / _long_f16, UNIIR_DT_F16 GEMMs); the residual stream, the norm statistics,
visual.proj's output, the final norm, the mean pool and the embedding stay fp32.  Forward only: no stash, no dropout.

fusion_forward_f32 (CLIPFeatureFusion.precision = "fp32"): the eval-mode embedding forward in fp32 on the fp32 masters of both stores,
a launch sequence of its own (uniir_sgemm, uniir_attn_f32_rel_fwd); it does not go through the dtype16 argument."""
import math

import torch

from . import ops
from .clip_model import CONV, image_blocks_f32, text_blocks_f32
from .fp32_forward import layernorm_f32, linear_f32, rmsnorm_f32
from .resblocks import block_set_bytes, clip_block_names, tower_bwd, tower_fwd

T5_EPS = 1e-6
T5_DROPOUT = 0.1      # transformers T5Config default dropout_rate (clip_ff.py:82,90 build T5Config() without overriding it)
T5_BUCKETS, T5_MAXDIST = 32, 128


def t5_param_shapes(d_model, heads, d_kv=64, d_ff=2048, layers=2):
    """flat order: q, k, v weights adjacent -> one [3 inner, d_model] GEMM"""
    inner = heads * d_kv
    out = []
    for i in range(layers):
        a, f = f"block.{i}.layer.0.", f"block.{i}.layer.1."
        out += [(a + "SelfAttention.q.weight", (inner, d_model)), (a + "SelfAttention.k.weight", (inner, d_model)),
                (a + "SelfAttention.v.weight", (inner, d_model)), (a + "SelfAttention.o.weight", (d_model, inner))]
        if i == 0:
            out += [(a + "SelfAttention.relative_attention_bias.weight", (T5_BUCKETS, heads))]
        out += [(a + "layer_norm.weight", (d_model,)), (f + "DenseReluDense.wi.weight", (d_ff, d_model)),
                (f + "DenseReluDense.wo.weight", (d_model, d_ff)), (f + "layer_norm.weight", (d_model,))]
    out += [("final_layer_norm.weight", (d_model,))]
    return out


def rel_bucket_table(T):
    """bucket of every offset key - query in [-(T-1), T-1] (T5Attention._relative_position_bucket, bidirectional);
    integer host logic, same float32 log as transformers"""
    rel = torch.arange(-(T - 1), T)
    nb = T5_BUCKETS // 2
    n = rel.abs()
    max_exact = nb // 2
    large = max_exact + (torch.log(n.float().clamp_min(1) / max_exact) / math.log(T5_MAXDIST / max_exact) * (nb - max_exact)).long()
    large = torch.min(large, torch.full_like(large, nb - 1))
    return ((rel > 0).long() * nb + torch.where(n < max_exact, n, large)).to(torch.int32)


_TABLES = {}


def _table(T, dev):
    key = (T, str(dev))
    if key not in _TABLES:
        _TABLES[key] = rel_bucket_table(T).to(dev)
    return _TABLES[key]


def _rel_entry(which, T):
    """the resident kernels up to ops.ATT_RESIDENT_MAX tokens, the streaming ones above (ViT-L/14@336px: 77 + 577 = 654 fused tokens)"""
    return f"uniir_attention_rel_{which}" + ("_long" if T > ops.ATT_RESIDENT_MAX else "")


def _rms(st, x, name, R, D, out_f32=False, dtype16=torch.bfloat16):
    y16 = torch.empty(R, D, device=x.device, dtype=dtype16) if not out_f32 else None
    y32 = torch.empty(R, D, device=x.device, dtype=torch.float32) if out_f32 else None
    if dtype16 == torch.float16:          # the fp32 output too: the fp16 forward stays on its own entry point
        ops.rmsnorm_fwd(x, st.p(name), T5_EPS, out_bf16=y16, out_f32=y32, rows=R, width=D, x_stride=D, dtype16=dtype16)
        return y32 if out_f32 else y16
    ops.call("uniir_rmsnorm_fwd", x, D, st.p(name), y16, y32, R, D, T5_EPS)
    return y32 if out_f32 else y16


def _check_dtype16(what, dtype16, save, drop=None):
    """the fp16 forward keeps nothing for a backward and takes no dropout: anything else raises before a launch -> is it fp16?"""
    if dtype16 not in (torch.bfloat16, torch.float16):
        raise ValueError(f"dtype16 is torch.bfloat16 or torch.float16, not {dtype16!r}")
    if dtype16 == torch.float16:
        if save:
            raise RuntimeError(f"the fp16 {what} keeps nothing for a backward (save=True needs dtype16=torch.bfloat16)")
        if drop is not None:
            raise RuntimeError(f"the fp16 {what} is the eval-mode embedding path: no dropout (drop needs dtype16=torch.bfloat16)")
    return dtype16 == torch.float16


def t5_forward(st, prefix, x, M, T, heads, layers, save, drop=None, p=T5_DROPOUT, dtype16=torch.bfloat16):
    """x fp32 [M*T, D] (the concatenated tokens; overwritten by its dropped version in train mode) -> pooled fp32 [M, D]
    (+ stash).  drop: ops.DropSeeds in train mode, None in eval mode.
    dtype16 = torch.float16 (eval mode, save False, drop None; anything else raises before a launch): the same sequence with fp16
    buffers, the weights from st's fp16 shadow, uniir_rmsnorm_fwd_f16 and ops.attention_rel_fwd_f16"""
    half = _check_dtype16("T5 forward", dtype16, save, drop)
    w16 = st.w16h if half else st.w16
    R, D = x.shape
    inner = heads * 64
    dev = x.device
    table = _table(T, dev)
    rel = st.p(prefix + "block.0.layer.0.SelfAttention.relative_attention_bias.weight")
    saved = []
    p = p if drop is not None else 0.0
    nxt = (lambda: drop.next()) if p else (lambda: 0)
    s_in = nxt()
    if p:
        ops.dropout_f32(x, p, s_in, out_f32=x)

    def branch(x16, w, resid):
        """resid + dropout(x16 @ w^T)"""
        if not p:
            return ops.linear_fwd(x16, w, epilogue=ops.EPI_RESID_F32, resid=resid), 0
        t = ops.linear_fwd(x16, w, epilogue=ops.EPI_RESID_F32)
        sd = nxt()
        ops.dropout_f32(t, p, sd, resid=resid, out_f32=t)
        return t, sd

    for i in range(layers):
        a, f = f"{prefix}block.{i}.layer.0.", f"{prefix}block.{i}.layer.1."
        h1 = _rms(st, x, a + "layer_norm.weight", R, D, dtype16=dtype16)
        qkv = ops.linear_fwd(h1, w16(a + "SelfAttention.q.weight", (3 * inner, D)))
        sa = nxt()
        if half:
            ao, lse = ops.attention_rel_fwd_f16(qkv, rel, table, M, T, heads, 1.0)
        else:
            ao = torch.empty(R, inner, device=dev, dtype=torch.bfloat16)
            lse = torch.empty(M, heads, T, device=dev, dtype=torch.float32)
            ops.call(_rel_entry("fwd", T), qkv, ao, lse, rel, table, T5_BUCKETS, 1.0, M, T, heads, p, sa)
        x2, so = branch(ao, w16(a + "SelfAttention.o.weight"), x)
        h2 = _rms(st, x2, f + "layer_norm.weight", R, D, dtype16=dtype16)
        wi = w16(f + "DenseReluDense.wi.weight")
        ff = torch.empty(R, wi.shape[0], device=dev, dtype=dtype16)
        g = torch.empty(R, wi.shape[0], device=dev, dtype=dtype16)
        ops.linear_fwd(h2, wi, out=ff, epilogue=ops.EPI_BIAS_ACT, C2=g, act=ops.ACT_RELU)
        sg = nxt()
        if p:
            ops.dropout_bf16_(g, p, sg)
        xn, sf = branch(g, w16(f + "DenseReluDense.wo.weight"), x2)
        if save:
            saved.append((x, h1, qkv, ao, lse, x2, h2, ff, (sa, so, sg, sf)))
        x = xn
    y = _rms(st, x, prefix + "final_layer_norm.weight", R, D, out_f32=True, dtype16=dtype16)
    s_fin = nxt()
    if p:
        ops.dropout_f32(y, p, s_fin, out_f32=y)
    pooled = torch.empty(M, D, device=dev, dtype=torch.float32)
    ops.call("uniir_meanpool_fwd", y, pooled, M, T, D)
    stash = dict(saved=saved, xf=x, M=M, T=T, p=p, s_in=s_in, s_fin=s_fin) if save else None
    return pooled, stash


def t5_backward(st, prefix, dpooled, stash, heads, layers):
    """returns d(concatenated tokens) fp32 [M*T, D]; parameter gradients accumulate into st.g32"""
    M, T = stash["M"], stash["T"]
    xf = stash["xf"]
    R, D = xf.shape
    inner = heads * 64
    dev = xf.device
    G = st.grad_view
    table = _table(T, dev)
    rel_name = prefix + "block.0.layer.0.SelfAttention.relative_attention_bias.weight"
    dy = torch.empty(R, D, device=dev, dtype=torch.float32)
    ops.call("uniir_meanpool_bwd", dpooled.contiguous(), dy, M, T, D)
    p = stash["p"]
    if p:
        ops.dropout_f32(dy, p, stash["s_fin"], out_f32=dy)
    dx = torch.empty(R, D, device=dev, dtype=torch.float32)
    dxb = torch.empty(R, D, device=dev, dtype=torch.bfloat16)
    ops.call("uniir_rmsnorm_bwd", xf, D, st.p(prefix + "final_layer_norm.weight"), dy, 1, None, dx, D, dxb,
             G(prefix + "final_layer_norm.weight"), R, D, T5_EPS)
    del dy
    for i in reversed(range(layers)):
        a, f = f"{prefix}block.{i}.layer.0.", f"{prefix}block.{i}.layer.1."
        x, h1, qkv, ao, lse, x2, h2, ff, (sa, so, sg, sf) = stash["saved"][i]
        stash["saved"][i] = None
        if p:       # the feed-forward branch sees the masked gradient; dx (fp32) keeps the residual one
            ops.dropout_bf16_(dxb, p, sf)
        wi, wo = st.w16(f + "DenseReluDense.wi.weight"), st.w16(f + "DenseReluDense.wo.weight")
        g = torch.empty_like(ff)
        df = torch.empty_like(ff)
        ops.linear_dgrad(dxb, wo, out=df, aux=ff, act_out=g, act=ops.ACT_RELU)        # df = (dx @ Wo) * relu'(ff), g = relu(ff)
        if p:       # the ReLU-output mask: on the re-materialised activation and (it commutes with relu') on its gradient
            ops.dropout_bf16_(g, p, sg)
            ops.dropout_bf16_(df, p, sg)
        ops.linear_wgrad(dxb, g, G(f + "DenseReluDense.wo.weight"))
        ops.linear_wgrad(df, h2, G(f + "DenseReluDense.wi.weight"))
        dh = ops.linear_dgrad(df, wi)
        dx2 = torch.empty(R, D, device=dev, dtype=torch.float32)
        ops.call("uniir_rmsnorm_bwd", x2, D, st.p(f + "layer_norm.weight"), dh, 0, dx, dx2, D, dxb, G(f + "layer_norm.weight"),
                 R, D, T5_EPS)
        del ff, g, df, h2, x2
        if p:
            ops.dropout_bf16_(dxb, p, so)
        ops.linear_wgrad(dxb, ao, G(a + "SelfAttention.o.weight"))
        dao = ops.linear_dgrad(dxb, st.w16(a + "SelfAttention.o.weight"))
        dqkv = torch.empty_like(qkv)
        ops.call(_rel_entry("bwd", T), qkv, ao, dao, lse, dqkv, st.p(rel_name), table, T5_BUCKETS, 1.0, G(rel_name), M, T,
                 heads, p, sa)
        ops.linear_wgrad(dqkv, h1, G(a + "SelfAttention.q.weight", (3 * inner, D)))
        dh = ops.linear_dgrad(dqkv, st.w16(a + "SelfAttention.q.weight", (3 * inner, D)))
        ops.call("uniir_rmsnorm_bwd", x, D, st.p(a + "layer_norm.weight"), dh, 0, dx2, dx, D, dxb, G(a + "layer_norm.weight"),
                 R, D, T5_EPS)
        del qkv, ao, lse, h1, x, dx2
    if p:
        ops.dropout_f32(dx, p, stash["s_in"], out_f32=dx)
    return dx


# ------------------------------------------------------------------------------------------------------------
# towers without pooling
# ------------------------------------------------------------------------------------------------------------
def _recompute_from(model, which, save, M, R, W, heads, L):
    """recompute_from of a tower without pooling: CLIP.recompute_blocks recomputes every block, the meaning the switch has for the C
    towers (the act(f) stash decisions of those do not exist here).  Logged once per tower in CLIP.stash_log."""
    if not (save and model.recompute_blocks):
        return None
    if which not in model._recompute_logged:
        model._recompute_logged.add(which)
        n = block_set_bytes(R, W, heads)
        model.stash_log.append(f"{which} tower without pooling, {M} items: block recomputation ON (recompute_blocks): block inputs only "
                               f"({L} x {4 * R * W} bytes) and one shared set of {n} bytes ({n / 2**30:.1f} GiB) that every block is "
                               f"rebuilt into; act(f) stash not applicable")
    return 0


def vision_tokens_fwd(model, image, save, dtype16=torch.bfloat16):
    """clip_ff.py:35-59 -> fp32 [M*T, E] = ln_post(all tokens) @ proj.  dtype16 = torch.float16 (save False): fp16 patches, blocks
    and ln_post output from the fp16 copies of the weights (the store's half_shadow()); the tokens stay fp32 (EPI_F32)"""
    half = _check_dtype16("vision tower", dtype16, save)
    cfg, st = model.cfg, model._flat
    dev = image.device
    M = image.shape[0]
    W, P, L, res, E = cfg["vision_width"], cfg["vision_patch_size"], cfg["vision_layers"], cfg["image_resolution"], cfg["embed_dim"]
    G_ = (res // P) ** 2
    T = G_ + 1
    heads = W // 64
    p32 = st.p
    patches = torch.empty(M * G_, model.kpad, device=dev, dtype=dtype16)
    ops.call("uniir_patchify_f16" if half else "uniir_patchify", image.float().contiguous(), patches, M, res, P, model.kpad)
    po = ops.linear_fwd(patches, st.padded16h(CONV) if half else st.padded16(CONV))
    x0 = torch.empty(M * T, W, device=dev, dtype=torch.float32)
    ops.call("uniir_vit_assemble_f16" if half else "uniir_vit_assemble", po, p32("visual.class_embedding"),
             p32("visual.positional_embedding"), x0, M, T, W)
    del po
    x = torch.empty(M * T, W, device=dev, dtype=torch.float32)
    ops.layernorm_fwd(x0, p32("visual.ln_pre.weight"), p32("visual.ln_pre.bias"), out_f32=x, rows=M * T, width=W)
    x, saved = tower_fwd(st, lambda i: clip_block_names("visual.transformer", i), L, x, M, T, W, heads, False, save,
                         recompute_from=_recompute_from(model, "image", save, M, M * T, W, heads, L), dtype16=dtype16)
    ln = ops.layernorm_fwd(x, p32("visual.ln_post.weight"), p32("visual.ln_post.bias"), rows=M * T, width=W, dtype16=dtype16)
    tok = torch.empty(M * T, E, device=dev, dtype=torch.float32)
    ops.gemm(ln, (st.w16h if half else st.w16)("visual.proj"), tok, M * T, E, W, W, E, E, b_tmaj=True, epilogue=ops.EPI_F32,
             dtype=ops.DT_F16 if half else ops.DT_BF16)
    stash = dict(patches=patches, x0=x0, saved=saved, xf=x, ln=ln, M=M, T=T) if save else None
    return tok, T, stash


def vision_tokens_bwd(model, dtok, stash):
    cfg, st = model.cfg, model._flat
    M, T = stash["M"], stash["T"]
    W, P, L, E = cfg["vision_width"], cfg["vision_patch_size"], cfg["vision_layers"], cfg["embed_dim"]
    R, dev, heads = M * T, dtok.device, W // 64
    p32, G = st.p, st.grad_view
    d16 = torch.empty(R, E, device=dev, dtype=torch.bfloat16)
    ops.call("uniir_cast_f32_to_bf16", dtok.contiguous(), d16, d16.numel())
    # dproj[W,E] += ln^T @ dtok ; dln[R,W] = dtok @ proj^T
    ops.gemm(stash["ln"], d16, G("visual.proj"), W, E, R, W, E, E, a_tmaj=True, b_tmaj=True,
             epilogue=ops.EPI_ATOMIC_F32, k_splits=ops.wgrad_splits(R, ((W + 255) // 256) * ((E + 255) // 256)))
    dln = torch.empty(R, W, device=dev, dtype=torch.bfloat16)
    ops.gemm(d16, st.w16("visual.proj"), dln, R, W, E, E, E, W)
    dxb = torch.empty(R, W, device=dev, dtype=torch.bfloat16)
    dx = ops.layernorm_bwd(stash["xf"], p32("visual.ln_post.weight"), dln, G("visual.ln_post.weight"),
                           G("visual.ln_post.bias"), dx_bf16=dxb, rows=R, width=W)
    dx = tower_bwd(st, lambda i: clip_block_names("visual.transformer", i), L, dx, dxb, stash["saved"], M, T, W, heads, False,
                   block_done=model.block_done("visual.transformer"))
    dx0 = ops.layernorm_bwd(stash["x0"], p32("visual.ln_pre.weight"), dx, G("visual.ln_pre.weight"),
                            G("visual.ln_pre.bias"), rows=R, width=W)
    dpo = torch.empty(M * (T - 1), W, device=dev, dtype=torch.bfloat16)
    ops.call("uniir_vit_assemble_bwd", dx0, dpo, G("visual.class_embedding"),
             G("visual.positional_embedding"), M, T, W)
    dconv = st.padded_grad(CONV).zero_()
    ops.linear_wgrad(dpo, stash["patches"], dconv)
    ops.call("uniir_unpad_add", dconv, G(CONV), W, 3 * P * P, model.kpad)


def text_tokens_fwd(model, text, save, dtype16=torch.bfloat16):
    """clip_ff.py:148-156 -> fp32 [M*77, W] = ln_final(all tokens).  dtype16 = torch.float16 (save False): the causal blocks in fp16"""
    _check_dtype16("text tower", dtype16, save)
    cfg, st = model.cfg, model._flat
    dev = text.device
    M = text.shape[0]
    W, L, T, heads = cfg["transformer_width"], cfg["transformer_layers"], cfg["context_length"], cfg["transformer_heads"]
    p32 = st.p
    x = torch.empty(M * T, W, device=dev, dtype=torch.float32)
    eot = torch.empty(M, device=dev, dtype=torch.int32)
    ops.call("uniir_text_embed", text, p32("token_embedding.weight"), p32("positional_embedding"), x, eot, M, T, W,
             cfg["vocab_size"])
    x, saved = tower_fwd(st, lambda i: clip_block_names("transformer", i), L, x, M, T, W, heads, True, save,
                         recompute_from=_recompute_from(model, "text", save, M, M * T, W, heads, L), dtype16=dtype16)
    tok = torch.empty(M * T, W, device=dev, dtype=torch.float32)
    ops.layernorm_fwd(x, p32("ln_final.weight"), p32("ln_final.bias"), out_f32=tok, rows=M * T, width=W)
    stash = dict(text=text, saved=saved, xf=x, M=M, T=T) if save else None
    return tok, T, stash


def text_tokens_bwd(model, dtok, stash):
    cfg, st = model.cfg, model._flat
    M, T = stash["M"], stash["T"]
    W, L, heads = cfg["transformer_width"], cfg["transformer_layers"], cfg["transformer_heads"]
    R, dev = M * T, dtok.device
    p32, G = st.p, st.grad_view
    dxb = torch.empty(R, W, device=dev, dtype=torch.bfloat16)
    dx = ops.layernorm_bwd(stash["xf"], p32("ln_final.weight"), dtok.contiguous(), G("ln_final.weight"),
                           G("ln_final.bias"), dx_bf16=dxb, rows=R, width=W)
    dx = tower_bwd(st, lambda i: clip_block_names("transformer", i), L, dx, dxb, stash["saved"], M, T, W, heads, True,
                   block_done=model.block_done("transformer"))
    ops.call("uniir_text_embed_bwd", stash["text"], dx, G("token_embedding.weight"),
             G("positional_embedding"), M, T, W, cfg["vocab_size"])


# ------------------------------------------------------------------------------------------------------------
# fp32 forward (CLIPFeatureFusion.precision = "fp32"): the reference's model.float() embedding forward on the fp32 launch layer
# (fp32_forward.py).  The towers without pooling are clip_model's fp32 blocks followed by ln_post + visual.proj / ln_final on every
# token; the T5 stack adds the fp32 relative-bias attention uniir_attn_f32_rel_fwd (csrc/fp32_path.hip).  Both stores' fp32 masters are
# read directly.  Forward only, eval mode: no stash, no dropout.
# ------------------------------------------------------------------------------------------------------------
def t5_forward_f32(st, prefix, x, M, T, heads, layers):
    """x fp32 [M*T, D] (the concatenated tokens) -> pooled fp32 [M, D]: t5_forward's eval-mode sequence in fp32"""
    R, D = x.shape
    inner = heads * 64
    table = _table(T, x.device)
    rel = st.p(prefix + "block.0.layer.0.SelfAttention.relative_attention_bias.weight")
    for i in range(layers):
        a, f = f"{prefix}block.{i}.layer.0.", f"{prefix}block.{i}.layer.1."
        qkv = linear_f32(rmsnorm_f32(x, st.p(a + "layer_norm.weight"), T5_EPS), st.p(a + "SelfAttention.q.weight", (3 * inner, D)))
        ao = torch.empty(R, inner, device=x.device, dtype=torch.float32)
        ops.call("uniir_attn_f32_rel_fwd", qkv, ao, rel, table, T5_BUCKETS, 1.0, M, T, heads)
        x = linear_f32(ao, st.p(a + "SelfAttention.o.weight"), resid=x)
        g = linear_f32(rmsnorm_f32(x, st.p(f + "layer_norm.weight"), T5_EPS), st.p(f + "DenseReluDense.wi.weight"), act=ops.ACT_RELU)
        x = linear_f32(g, st.p(f + "DenseReluDense.wo.weight"), resid=x)
    pooled = torch.empty(M, D, device=x.device, dtype=torch.float32)
    ops.call("uniir_meanpool_fwd", rmsnorm_f32(x, st.p(prefix + "final_layer_norm.weight"), T5_EPS), pooled, M, T, D)
    return pooled


def vision_tokens_f32(model, image):
    """vision_tokens_fwd in fp32 -> fp32 [M*T, E] = ln_post(all tokens) @ proj, and T"""
    p32 = model._flat.p
    x, T = image_blocks_f32(model, image)
    ln = layernorm_f32(x, p32("visual.ln_post.weight"), p32("visual.ln_post.bias"))
    return linear_f32(ln, p32("visual.proj"), w_kn=True), T          # ln @ proj, proj [W, E]


def text_tokens_f32(model, text):
    """text_tokens_fwd in fp32 -> fp32 [M*77, W] = ln_final(all tokens), and the context length"""
    x, _, T = text_blocks_f32(model, text)
    return layernorm_f32(x, model._flat.p("ln_final.weight"), model._flat.p("ln_final.bias")), T


def fusion_forward_f32(owner, text, image):
    """FusionFn.forward in fp32 (no autograd node: the caller has refused grad mode)"""
    ttok, Tt = text_tokens_f32(owner.clip_model, text)
    itok, Ti = vision_tokens_f32(owner.clip_model, image)
    M, D = text.shape[0], ttok.shape[1]
    x = torch.cat([ttok.view(M, Tt, D), itok.view(M, Ti, D)], dim=1).view(M * (Tt + Ti), D)     # a copy, no arithmetic
    return t5_forward_f32(owner._t5, "", x, M, Tt + Ti, owner.t5_heads, owner.t5_layers_n)


class FusionFn(torch.autograd.Function):
    """(clip module, T5 store, text int32 [M,77], image [M,3,H,W]) -> fused embedding fp32 [M, D]"""

    @staticmethod
    def forward(ctx, owner, text, image, anchor):
        save = bool(ctx.needs_input_grad[3])
        clip, st = owner.clip_model, owner._t5
        # the owner's precision (CLIPFeatureFusion._embed_mode() has refused what fp16 cannot serve): "fp16" = the embedding forward
        dt = torch.float16 if owner.precision == "fp16" else torch.bfloat16
        ttok, Tt, tst = text_tokens_fwd(clip, text, save, dtype16=dt)
        itok, Ti, ist = vision_tokens_fwd(clip, image, save, dtype16=dt)
        M, D = text.shape[0], ttok.shape[1]
        x = torch.cat([ttok.view(M, Tt, D), itok.view(M, Ti, D)], dim=1).view(M * (Tt + Ti), D)     # a copy, no arithmetic
        del ttok, itok
        drop = ops.DropSeeds() if owner.training and owner.t5_dropout > 0 else None
        pooled, fst = t5_forward(st, "", x, M, Tt + Ti, owner.t5_heads, owner.t5_layers_n, save, drop=drop,
                                 p=owner.t5_dropout, dtype16=dt)
        ctx.owner, ctx.stashes, ctx.dims = owner, (tst, ist, fst), (M, Tt, Ti, D)
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        owner = ctx.owner
        tst, ist, fst = ctx.stashes
        ctx.stashes = None
        M, Tt, Ti, D = ctx.dims
        dx = t5_backward(owner._t5, "", dpooled, fst, owner.t5_heads, owner.t5_layers_n).view(M, Tt + Ti, D)
        reducer = getattr(owner.clip_model, "_grad_reducer", None)
        if reducer is not None:        # the T5 gradients are final: their all-reduce overlaps the two tower backwards
            reducer.reduce_extra(owner._t5.g32)
        dt = dx[:, :Tt].contiguous().view(M * Tt, D)
        di = dx[:, Tt:].contiguous().view(M * Ti, D)
        del dx
        text_tokens_bwd(owner.clip_model, dt, tst)
        vision_tokens_bwd(owner.clip_model, di, ist)
        return None, None, None, None
