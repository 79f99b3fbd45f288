"""MI355X-native BLIP feature-fusion model: BLIP ViT + MED BERT with cross-attention,
momentum encoders, feature queues and the soft-target contrastive loss, behind the module surface of the reference's
src/models/uniir_blip/blip_featurefusion/blip_ff.py:19-310 (same constructor arguments, attribute names, state-dict
keys `visual_encoder.* / text_encoder.* / visual_encoder_m.* / text_encoder_m.* / temp / query_queue / cand_queue /
idx_queue / new_ptr_queue`, forward(batch, alpha, encode_mbeir_batch)).

All arithmetic is in libuniir_hip.so; this file is the launch sequence, the flat parameter stores and the activation
stash.  Differences from the reference, stated once:
  * bf16 MFMA GEMMs with fp32 accumulation / fp32 LayerNorm, softmax statistics, residual stream, loss (the reference
    runs fp16 autocast); no GradScaler is needed; the eval-mode embedding forward alone also runs on fp16 operands
    (BLIPFeatureFusion.precision = "fp16", the reference embedder's autocast) or in fp32 (precision = "fp32", its model.float()
    forward: vit_forward_f32 / bert_forward_f32);
  * train mode applies the reference's dropout sites -- BERT hidden / attention-probability dropout 0.1 (med.py:84,
    175,198,212,341; online and momentum encoders alike, both are in train mode) and DropPath of ViT-large (vit.py:79-80,
    blip.py:249-254) -- with counter-based masks regenerated in backward (ops.DropSeeds); the masks are a different random
    stream than torch's, so only the distribution matches; eval mode (and a config with zero rates) is deterministic;
  * the BERT padding mask must be a prefix mask (tokenizer padding="max_length"), it travels as one key length per row;
  * hard negatives (blip_ff.py:127-131,159-170,233-246) are supported; like the reference their momentum features are
    used un-normalised and a host coin flip decides what is enqueued.
"""
import functools
import json
import logging

import torch
from torch import nn

from . import _lib, comm, ops
from .flat_store import FlatStore, patch_kpad
from .fp32_forward import attention_f32, layernorm_f32, linear_f32, patch_tokens_f32, tower_fwd_f32
from .precision import check_mode, embed_mode, env_flag
from .resblocks import tower_bwd, tower_fwd

VIT_CONFIGS = {   # src/models/uniir_blip/backbone/blip.py:229-255 (create_vit)
    "base": dict(patch_size=16, embed_dim=768, depth=12, num_heads=12, drop_path_rate=0.0),
    "large": dict(patch_size=16, embed_dim=1024, depth=24, num_heads=16, drop_path_rate=0.1),
}
MED_DEFAULT = dict(hidden_size=768, intermediate_size=3072, layer_norm_eps=1e-12, max_position_embeddings=512,
                   num_attention_heads=12, num_hidden_layers=12, vocab_size=30524, hidden_dropout_prob=0.1,
                   attention_probs_dropout_prob=0.1)   # backbone/configs/med_config.json
VIT_EPS = 1e-6
CONV = "patch_embed.proj.weight"          # below a ViT's prefix: the tensor its store keeps [D, kpad] copies of (FlatStore.add_padded)


# ------------------------------------------------------------------------------------------------------------
# names
# ------------------------------------------------------------------------------------------------------------
def vit_param_shapes(cfg, img_size):
    D, P = cfg["embed_dim"], cfg["patch_size"]
    T = (img_size // P) ** 2 + 1
    out = [("cls_token", (1, 1, D)), ("pos_embed", (1, T, D)), ("patch_embed.proj.weight", (D, 3, P, P)),
           ("patch_embed.proj.bias", (D,))]
    for i in range(cfg["depth"]):
        b = f"blocks.{i}."
        out += [(b + "norm1.weight", (D,)), (b + "norm1.bias", (D,)), (b + "attn.qkv.weight", (3 * D, D)),
                (b + "attn.qkv.bias", (3 * D,)), (b + "attn.proj.weight", (D, D)), (b + "attn.proj.bias", (D,)),
                (b + "norm2.weight", (D,)), (b + "norm2.bias", (D,)), (b + "mlp.fc1.weight", (4 * D, D)),
                (b + "mlp.fc1.bias", (4 * D,)), (b + "mlp.fc2.weight", (D, 4 * D)), (b + "mlp.fc2.bias", (D,))]
    out += [("norm.weight", (D,)), ("norm.bias", (D,))]
    return out


def bert_param_shapes(cfg, enc_width, pooler=True):
    """flat order: query/key/value weights (and biases) adjacent, so one [3W,W] (self) / [2W,enc] (cross) GEMM serves them"""
    W, I = cfg["hidden_size"], cfg["intermediate_size"]
    out = [("embeddings.word_embeddings.weight", (cfg["vocab_size"], W)),
           ("embeddings.position_embeddings.weight", (cfg["max_position_embeddings"], W)),
           ("embeddings.LayerNorm.weight", (W,)), ("embeddings.LayerNorm.bias", (W,))]
    for i in range(cfg["num_hidden_layers"]):
        b = f"encoder.layer.{i}."
        s, c = b + "attention.self.", b + "crossattention.self."
        out += [(s + "query.weight", (W, W)), (s + "key.weight", (W, W)), (s + "value.weight", (W, W)),
                (s + "query.bias", (W,)), (s + "key.bias", (W,)), (s + "value.bias", (W,)),
                (b + "attention.output.dense.weight", (W, W)), (b + "attention.output.dense.bias", (W,)),
                (b + "attention.output.LayerNorm.weight", (W,)), (b + "attention.output.LayerNorm.bias", (W,)),
                (c + "query.weight", (W, W)), (c + "query.bias", (W,)),
                (c + "key.weight", (W, enc_width)), (c + "value.weight", (W, enc_width)),
                (c + "key.bias", (W,)), (c + "value.bias", (W,)),
                (b + "crossattention.output.dense.weight", (W, W)), (b + "crossattention.output.dense.bias", (W,)),
                (b + "crossattention.output.LayerNorm.weight", (W,)), (b + "crossattention.output.LayerNorm.bias", (W,)),
                (b + "intermediate.dense.weight", (I, W)), (b + "intermediate.dense.bias", (I,)),
                (b + "output.dense.weight", (W, I)), (b + "output.dense.bias", (W,)),
                (b + "output.LayerNorm.weight", (W,)), (b + "output.LayerNorm.bias", (W,))]
    if pooler:
        out += [("pooler.dense.weight", (W, W)), ("pooler.dense.bias", (W,))]
    return out


def _vit_blk_names(prefix, i):
    b = f"{prefix}blocks.{i}."
    return dict(wqkv=b + "attn.qkv.weight", bqkv=b + "attn.qkv.bias", wo=b + "attn.proj.weight", bo=b + "attn.proj.bias",
                ln1w=b + "norm1.weight", ln1b=b + "norm1.bias", wfc=b + "mlp.fc1.weight", bfc=b + "mlp.fc1.bias",
                wproj=b + "mlp.fc2.weight", bproj=b + "mlp.fc2.bias", ln2w=b + "norm2.weight", ln2b=b + "norm2.bias")


def _attach(root, dotted, param):
    mod = root
    parts = dotted.split(".")
    for part in parts[:-1]:
        if part not in mod._modules:
            mod.add_module(part, nn.Module())
        mod = mod._modules[part]
    mod.register_parameter(parts[-1], param)


# ------------------------------------------------------------------------------------------------------------
# launch sequences
# ------------------------------------------------------------------------------------------------------------
def vit_recompute_from(depth, vit_grad_ckpt, vit_ckpt_layer):
    """the first ViT block whose intermediates are recomputed in the backward, from the reference's two configuration keys: it
    checkpoints the blocks i >= depth - ckpt_layer when use_grad_checkpointing is set (backbone/vit.py:230), so vit_ckpt_layer: 0
    with the flag on recomputes nothing, like there.  Returns depth (nothing recomputed) without the flag.
    The reference checkpoints a block's attention and MLP branches separately (two checkpoints per block, each keeping its input);
    here the unit is the whole block, which keeps less: the fp32 block input alone (resblocks.tower_fwd's recompute_from)."""
    if not vit_grad_ckpt:
        return depth
    return depth - min(max(int(vit_ckpt_layer), 0), depth)


def vit_forward(st, prefix, cfg, img_size, images, save, drop=None, recompute_from=None, dtype16=torch.bfloat16):
    """src/models/uniir_blip/backbone/vit.py:196-221 -> bf16 tokens [M*T, D] (after the final norm) + stash.
    dtype16 = torch.float16 (forward only: save False): patches, activations and the returned tokens are fp16, the weights come from
    st's fp16 shadow (FlatStore.w16h, and padded16h for the patch-embedding weight); the residual stream, the LayerNorm
    statistics and every accumulation stay fp32.  Three more mantissa bits in every operand, the same MFMA rate.
    drop (ops.DropSeeds, train mode): DropPath with rates linspace(0, drop_path_rate, depth) (vit.py:167), one Bernoulli
    draw per item and residual branch from torch's CPU generator.
    recompute_from: blocks from this one on keep only their input and are rebuilt in vit_backward (vit_recompute_from); the
    stash carries what each block kept, so vit_backward needs no argument for it"""
    D, P, depth = cfg["embed_dim"], cfg["patch_size"], cfg["depth"]
    M, dev = images.shape[0], images.device
    G = (img_size // P) ** 2
    T = G + 1
    heads = cfg["num_heads"]
    half = dtype16 == torch.float16
    conv16 = (st.padded16h if half else st.padded16)(prefix + CONV)
    kpad = conv16.shape[1]
    patches = torch.empty(M * G, kpad, device=dev, dtype=dtype16)
    ops.call("uniir_patchify_f16" if half else "uniir_patchify", images.float().contiguous(), patches, M, img_size, P, kpad)
    po = ops.linear_fwd(patches, conv16, st.p(prefix + "patch_embed.proj.bias"))
    x0 = torch.empty(M * T, D, device=dev, dtype=torch.float32)
    ops.call("uniir_vit_assemble_f16" if half else "uniir_vit_assemble", po, st.p(prefix + "cls_token"), st.p(prefix + "pos_embed"),
             x0, M, T, D)
    del po
    rowscale = None
    if drop is not None and cfg.get("drop_path_rate", 0.0) > 0 and depth > 1:
        keep = 1.0 - torch.linspace(0, cfg["drop_path_rate"], depth).view(depth, 1, 1)
        rowscale = (torch.floor(keep + torch.rand(depth, 2, M)) / keep).to(dev)
    x, saved = tower_fwd(st, lambda i: _vit_blk_names(prefix, i), depth, x0, M, T, D, heads, False, save, eps=VIT_EPS,
                         act=ops.ACT_GELU_ERF, rowscale=rowscale, recompute_from=recompute_from, dtype16=dtype16)
    tok = ops.layernorm_fwd(x, st.p(prefix + "norm.weight"), st.p(prefix + "norm.bias"), VIT_EPS, rows=M * T, width=D,
                            dtype16=dtype16)
    stash = dict(patches=patches, x=x, saved=saved, M=M, T=T, rowscale=rowscale, recompute_from=recompute_from) if save else None
    return tok, T, stash


def vit_backward(st, prefix, cfg, dtok, stash):
    """dtok fp32 [M*T, D]: gradient w.r.t. the normed tokens; parameter gradients accumulate into st.g32"""
    D, P, depth, heads = cfg["embed_dim"], cfg["patch_size"], cfg["depth"], cfg["num_heads"]
    M, T = stash["M"], stash["T"]
    R, dev = M * T, dtok.device
    dxb = torch.empty(R, D, device=dev, dtype=torch.bfloat16)
    dx = ops.layernorm_bwd(stash["x"], st.p(prefix + "norm.weight"), dtok, st.grad_view(prefix + "norm.weight"),
                           st.grad_view(prefix + "norm.bias"), VIT_EPS, dx_bf16=dxb, rows=R, width=D)
    dx = tower_bwd(st, lambda i: _vit_blk_names(prefix, i), depth, dx, dxb, stash["saved"], M, T, D, heads, False, eps=VIT_EPS,
                   act=ops.ACT_GELU_ERF, rowscale=stash["rowscale"])
    G = T - 1
    dpo = torch.empty(M * G, D, device=dev, dtype=torch.bfloat16)
    ops.call("uniir_vit_assemble_bwd", dx, dpo, st.grad_view(prefix + "cls_token"), st.grad_view(prefix + "pos_embed"),
             M, T, D)
    ops.call("uniir_colsum_bf16", dpo, D, st.grad_view(prefix + "patch_embed.proj.bias"), M * G, D)
    dconv = st.padded_grad(prefix + CONV).zero_()
    ops.linear_wgrad(dpo, stash["patches"], dconv)
    ops.call("uniir_unpad_add", dconv, st.grad_view(prefix + CONV), D, 3 * P * P, dconv.shape[1])


class TextPack:
    """The rows of a padded [M, L] token batch up to each caption's valid length, packed back to back.  The
    reference runs BERT on all L positions and masks the padded KEYS with (1 - m) * -10000 (med.py:687-688: exp underflows to an
    exact 0 in fp32), and only token 0 reaches pooler_output (blip_ff.py:82-116) -- so the rows behind a caption's last valid token
    never influence a result and carry exactly zero gradient.  Running the 12 layers on the live rows only changes no live row's
    value (the attention kernels take per-item row ranges, uniir_attention_fwd_rows; dropout masks are drawn at the dense
    coordinates); at the bench's lengths U{5..100} of 100 it drops 47 % of BERT's rows.
    row_off int32 [M + 1] (device), row_map int32 [R] (device: the dense row m * L + t of every packed row), R (host)."""

    def __init__(self, lens_host, L, dev):
        lens = lens_host.to(torch.int64).flatten()
        M = lens.numel()
        off = torch.zeros(M + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(lens, 0)
        self.R, self.M, self.L = int(off[-1]), M, int(L)
        first = torch.repeat_interleave(torch.arange(M, dtype=torch.int64) * L - off[:-1], lens)      # dense row - packed row
        row_map = first + torch.arange(self.R, dtype=torch.int64)
        self.row_off = off.to(torch.int32).to(dev, non_blocking=True)
        self.row_map = row_map.to(torch.int32).to(dev, non_blocking=True)

    @staticmethod
    def build(key_len, L, dev=None):
        """from the key lengths: a host tensor (dev = where the rows live), or the device tensor (one device -> host read; the
        prefix-mask check of _text_inputs has synchronised already).  None when packing is pointless (every caption full) or
        impossible (an empty caption)"""
        dev = key_len.device if dev is None else dev
        lens = key_len.detach().to("cpu")
        if lens.numel() == 0 or int(lens.min()) < 1 or int(lens.max()) > L or int(lens.sum()) == lens.numel() * L:
            return None
        return TextPack(lens, L, dev)


class _BertCall:
    """What one bert_forward / bert_backward call knows about itself: the sizes, the rows (dense or packed), the dropout rates and the
    weight shadow of its 16-bit type.  Built once in the forward and again from the stash in the backward."""

    def __init__(self, st, prefix, cfg, M, L, Ti, key_len, img16, pack, ph, pa, cross, drop=None, dtype16=torch.bfloat16):
        self.st, self.prefix, self.cross, self.drop, self.dtype16 = st, prefix, cross, drop, dtype16
        self.W, self.I, self.eps = cfg["hidden_size"], cfg["intermediate_size"], cfg["layer_norm_eps"]
        self.heads, self.layers, self.vocab = cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["vocab_size"]
        self.M, self.L, self.Ti, self.key_len, self.img16, self.pack, self.ph, self.pa = M, L, Ti, key_len, img16, pack, ph, pa
        self.half, self.dev = dtype16 == torch.float16, key_len.device
        self.w16 = st.w16h if self.half else st.w16
        self.R = pack.R if pack is not None else M * L
        self.roff = pack.row_off if pack is not None else None
        self.rmap = pack.row_map if pack is not None else None
        # attention on dense rows (padding mask key_len) or on the packed rows (the item's own length is its key count)
        self.self_kw = dict(key_len=key_len) if pack is None else dict(row_off=self.roff, kv_packed=True)
        self.cross_kw = {} if pack is None else dict(row_off=self.roff, kv_packed=False)
        self.out_rows = {} if pack is None else dict(rows=self.R)          # the forward allocates its packed output by this

    @classmethod
    def of_stash(cls, st, prefix, cfg, stash, cross):
        return cls(st, prefix, cfg, stash["M"], stash["L"], stash["Ti"], stash["key_len"], stash["img16"], stash.get("pack"),
                   stash["ph"], stash["pa"], cross)

    def f32(self, *shape, zero=False):
        return (torch.zeros if zero else torch.empty)(*shape, device=self.dev, dtype=torch.float32)

    def b16(self, *shape, zero=False):
        """a 16-bit activation: bf16, or fp16 in the fp16 forward"""
        return (torch.zeros if zero else torch.empty)(*shape, device=self.dev, dtype=self.dtype16)

    def seed(self, p):
        """the next dropout seed of the pass for a site with rate p (0: the site launches nothing and draws nothing)"""
        return self.drop.next() if p else 0

    def attention(self, name, *args, seed, at=None, **kw):
        """the forward attention `name` (ops.attention_fwd_ex / ops.onequery_fwd) in this call's 16-bit type: the fp16 wrappers take no
        dropout arguments, the bf16 ones get the rate, the seed and `at` (the coordinates of a one-query call's dropout)"""
        if self.half:
            return getattr(ops, name + "_f16")(*args, **kw)
        return getattr(ops, name)(*args, drop_p=self.pa, drop_seed=seed, **(at or {}), **kw)

    def ln2(self, x, wname, n):
        """post-LN sublayer output in both precisions: fp32 for the next residual, bf16 (fp16 in the fp16 forward, through
        uniir_layernorm_fwd_f16) for the next GEMM"""
        o32, o16 = self.f32(n, self.W), self.b16(n, self.W)
        ops.layernorm_fwd(x, self.st.p(wname + "weight"), self.st.p(wname + "bias"), self.eps, out_bf16=o16, out_f32=o32, rows=n,
                          width=self.W)
        return o32, o16

    def out_dense(self, x16, name, resid, row_map):
        """dense -> dropout -> + residual (BertSelfOutput / BertOutput, med.py:196-200,339-343), pre-LayerNorm sum"""
        w, bias = self.w16(name + "weight"), self.st.p(name + "bias")
        if not self.ph:
            return ops.linear_fwd(x16, w, bias, epilogue=ops.EPI_RESID_F32, resid=resid), 0
        t = ops.linear_fwd(x16, w, bias, epilogue=ops.EPI_RESID_F32)
        sd = self.drop.next()
        ops.dropout_f32(t, self.ph, sd, resid=resid, out_f32=t, row_map=row_map)
        return t, sd


class _AllRows:
    """A layer on all R rows of the batch, dense [M * L] or packed: the general attention, the residual stream as it is."""

    def __init__(self, cx, full_layers):
        self.cx, self.n, self.row_map = cx, cx.R, cx.rmap
        # gelu's output [R, I]: one buffer serves every full layer of the call (nothing keeps it after output.dense has read it)
        self.g = cx.b16(cx.R, cx.I) if full_layers else None

    def g_buffer(self):
        return self.g

    def take(self, h32):
        return h32

    def spread(self, d):
        return d

    def self_fwd(self, qkv, seed):
        cx, W = self.cx, self.cx.W
        return cx.attention("attention_fwd_ex", qkv, 3 * W, qkv[:, W:], qkv[:, 2 * W:], 3 * W, cx.M, cx.L, cx.L, cx.heads, seed=seed,
                            **cx.self_kw, **cx.out_rows) + ({},)

    def cross_fwd(self, cq, ckv, seed):
        cx, W = self.cx, self.cx.W
        return cx.attention("attention_fwd_ex", cq, W, ckv, ckv[:, W:], 2 * W, cx.M, cx.L, cx.Ti, cx.heads, seed=seed, **cx.cross_kw,
                            **cx.out_rows)

    def self_bwd(self, sv, dao, seed):
        cx, W, qkv = self.cx, self.cx.W, sv["qkv"]
        dqkv = cx.b16(self.n, 3 * W)
        ops.attention_bwd_ex(qkv, 3 * W, qkv[:, W:], qkv[:, 2 * W:], 3 * W, sv["ao"], dao, sv["lse1"], dqkv, 3 * W, dqkv[:, W:],
                             dqkv[:, 2 * W:], 3 * W, cx.M, cx.L, cx.L, cx.heads, drop_p=cx.pa, drop_seed=seed, **cx.self_kw)
        return dqkv

    def cross_bwd(self, sv, dco, dcq, dckv, seed):
        cx, W, ckv = self.cx, self.cx.W, sv["ckv"]
        ops.attention_bwd_ex(sv["cq"], W, ckv, ckv[:, W:], 2 * W, sv["co"], dco, sv["lse2"], dcq, W, dckv, dckv[:, W:], 2 * W, cx.M,
                             cx.L, cx.Ti, cx.heads, drop_p=cx.pa, drop_seed=seed, **cx.cross_kw)


class _ClassRows:
    """The last BERT layer when only the class row of every item leaves the encoder (blip_ff.py:82-116 reads pooler_output,
    blip_sf.py the class token): what that row needs from the other rows is their KEYS AND VALUES, so the q | k | v projection still
    runs on all R rows -- the same GEMM as in the full layer, so K | V have its bits, a dense BERT passes row m * L of that buffer as
    the query without a copy, and the backward's weight-gradient and d h32 products keep their shape -- and everything behind it on
    the M class rows: the one-query self-attention (ops.onequery_fwd with key_len or the packed rows), attention.output.dense +
    LayerNorm, the cross query, the one-query cross-attention over the Ti image tokens, its output dense + LayerNorm, the FFN and
    output.LayerNorm.  The dropout seeds are drawn in the full layer's order; attention dropout sits at the coordinates of query 0 of
    L (drop_tq = L, drop_q = 0), hidden dropout at the dense rows m * L (row_map).
    Backward: everything up to the self-attention runs on M rows; the one-query backward writes dk | dv of EVERY key row (exact zeros
    behind a dense item's key_len) and dq of the class rows into a zeroed [R, 3W] buffer -- the rows whose query gradient the full
    layer finds to be zero -- so the q | k | v weight gradient and d h32 = dqkv @ Wqkv + dt1 are the full layer's products; dt1 is
    scattered into zeroed R rows.
    take / spread are also how a full last layer's class rows leave the encoder and how their gradient comes back."""

    def __init__(self, cx):
        self.cx, self.n = cx, cx.M
        self.at = dict(drop_tq=cx.L, drop_q=0)

    @functools.cached_property
    def row_map(self):
        """int32: the DENSE row m * L of each of the M rows (the coordinates of hidden dropout)"""
        return torch.arange(self.n, device=self.cx.dev, dtype=torch.int32) * self.cx.L

    @functools.cached_property
    def cls(self):
        """the class token's row among the packed rows = the first row of every item, as an index tensor"""
        return self.cx.roff[:self.n].long()

    def g_buffer(self):
        return self.cx.b16(self.n, self.cx.I)

    def take(self, h32):
        cx = self.cx
        rows = cx.f32(self.n, cx.W)
        ops.call("uniir_gather_rows", h32, cx.roff, rows, cx.M, cx.L if cx.pack is None else 0, cx.W)
        return rows

    def spread(self, d):
        cx = self.cx
        out = cx.f32(cx.R, cx.W, zero=True)
        ops.call("uniir_scatter_rows", d, cx.roff, out, cx.M, cx.L if cx.pack is None else 0, cx.W)
        return out

    def self_fwd(self, qkv, seed):
        cx, W = self.cx, self.cx.W
        if cx.pack is None:
            q, q_ld, kw = qkv, cx.L * 3 * W, dict(key_len=cx.key_len)
        else:
            q, q_ld, kw = qkv[self.cls, :W], W, dict(kv_row_off=cx.roff)          # a copy of M rows
        return cx.attention("onequery_fwd", q, q_ld, qkv[:, W:], qkv[:, 2 * W:], 3 * W, cx.M, cx.L, cx.heads, seed=seed, at=self.at,
                            **kw) + (dict(pooled=True, q=q, q_ld=q_ld),)

    def cross_fwd(self, cq, ckv, seed):
        cx, W = self.cx, self.cx.W
        return cx.attention("onequery_fwd", cq, W, ckv, ckv[:, W:], 2 * W, cx.M, cx.Ti, cx.heads, seed=seed, at=self.at)

    def self_bwd(self, sv, dao, seed):
        cx, W, qkv = self.cx, self.cx.W, sv["qkv"]
        dqkv = cx.b16(cx.R, 3 * W, zero=True)
        if cx.pack is None:
            dq, kw = dqkv, dict(key_len=cx.key_len)
        else:
            dq, kw = cx.b16(self.n, W), dict(kv_row_off=cx.roff)
        ops.onequery_bwd(sv["q"], sv["q_ld"], qkv[:, W:], qkv[:, 2 * W:], 3 * W, sv["ao"], dao, sv["lse1"], dq, sv["q_ld"], dqkv[:, W:],
                         dqkv[:, 2 * W:], 3 * W, cx.M, cx.L, cx.heads, drop_p=cx.pa, drop_seed=seed, **self.at, **kw)
        if cx.pack is not None:
            dqkv[self.cls, :W] = dq          # a copy of M rows
        return dqkv

    def cross_bwd(self, sv, dco, dcq, dckv, seed):
        cx, W, ckv = self.cx, self.cx.W, sv["ckv"]
        ops.onequery_bwd(sv["cq"], W, ckv, ckv[:, W:], 2 * W, sv["co"], dco, sv["lse2"], dcq, W, dckv, dckv[:, W:], 2 * W, cx.M, cx.Ti,
                         cx.heads, drop_p=cx.pa, drop_seed=seed, **self.at)


def _layer_forward(cx, rows, i, h32, h16, save):
    """BertLayer i of med.py on `rows` (an _AllRows or a _ClassRows of cx): self-attention, cross-attention over the image tokens
    (mode "multimodal"), feed-forward, each closed by dense -> dropout -> + residual -> LayerNorm.  h32 / h16: the layer's input on
    all R rows.  -> the output on rows.n rows in fp32 and 16 bits, and what the backward needs (None without save)"""
    st, w16, W, n = cx.st, cx.w16, cx.W, rows.n
    b = f"{cx.prefix}encoder.layer.{i}."
    s, c = b + "attention.self.", b + "crossattention.self."
    qkv = ops.linear_fwd(h16, w16(s + "query.weight", (3 * W, W)), st.p(s + "query.bias", (3 * W,)))
    sa1 = cx.seed(cx.pa)
    ao, lse1, kept = rows.self_fwd(qkv, sa1)          # kept: what the backward of these rows needs beyond the tensors below
    t1, so1 = cx.out_dense(ao, b + "attention.output.dense.", rows.take(h32), rows.row_map)
    a32, a16 = cx.ln2(t1, b + "attention.output.LayerNorm.", n)
    cq = ckv = co = lse2 = t2 = None
    sa2 = so2 = 0
    if cx.cross:
        cq = ops.linear_fwd(a16, w16(c + "query.weight"), st.p(c + "query.bias"))
        ckv = ops.linear_fwd(cx.img16, w16(c + "key.weight", (2 * W, cx.img16.shape[1])), st.p(c + "key.bias", (2 * W,)))
        sa2 = cx.seed(cx.pa)
        co, lse2 = rows.cross_fwd(cq, ckv, sa2)
        t2, so2 = cx.out_dense(co, b + "crossattention.output.dense.", a32, rows.row_map)
        c32, c16 = cx.ln2(t2, b + "crossattention.output.LayerNorm.", n)
    else:
        c32, c16 = a32, a16
    f, g = cx.b16(n, cx.I), rows.g_buffer()
    ops.linear_fwd(c16, w16(b + "intermediate.dense.weight"), st.p(b + "intermediate.dense.bias"), out=f,
                   epilogue=ops.EPI_BIAS_ACT, C2=g, act=ops.ACT_GELU_ERF)
    t3, so3 = cx.out_dense(g, b + "output.dense.", c32, rows.row_map)
    sv = dict(h16=h16, qkv=qkv, ao=ao, lse1=lse1, t1=t1, a16=a16, cq=cq, ckv=ckv, co=co, lse2=lse2, t2=t2, c16=c16, f=f, t3=t3,
              seeds=(sa1, so1, sa2, so2, so3), **kept) if save else None
    return cx.ln2(t3, b + "output.LayerNorm.", n) + (sv,)


def _layer_backward(cx, rows, i, sv, do, dimg):
    """backward of _layer_forward on the same `rows`.  do fp32 [rows.n, W]: the gradient of the layer's output; dimg (cross-attention)
    accumulates the gradient of the image tokens.  -> d h32 fp32 [R, W], the gradient of the layer's input on all R rows"""
    st, G, W, I, n, eps, ph = cx.st, cx.st.grad_view, cx.W, cx.I, rows.n, cx.eps, cx.ph
    b = f"{cx.prefix}encoder.layer.{i}."
    s, c = b + "attention.self.", b + "crossattention.self."
    sa1, so1, sa2, so2, so3 = sv["seeds"]
    # ---- feed-forward sublayer: o = LN(g @ Wout^T + bout + c32), g = gelu(c16 @ Wi^T + bi)
    d16 = cx.b16(n, W)
    dt3 = ops.layernorm_bwd(sv["t3"], st.p(b + "output.LayerNorm.weight"), do, G(b + "output.LayerNorm.weight"),
                            G(b + "output.LayerNorm.bias"), eps, dx_bf16=d16, rows=n, width=W)
    if ph:      # the dense branch sees the masked gradient, the residual branch (dt3, fp32) the full one
        ops.dropout_bf16_(d16, ph, so3, row_map=rows.row_map)
    df, g = cx.b16(n, I), rows.g_buffer()
    ops.linear_dgrad(d16, st.w16(b + "output.dense.weight"), out=df, aux=sv["f"], act_out=g,
                     colsum=G(b + "intermediate.dense.bias"), act=ops.ACT_GELU_ERF)
    ops.linear_wgrad(d16, g, G(b + "output.dense.weight"), dbias=G(b + "output.dense.bias"))
    ops.linear_wgrad(df, sv["c16"], G(b + "intermediate.dense.weight"))
    dc = cx.f32(n, W)       # d c32 = df @ Wi + dt3 (the residual branch)
    ops.gemm(df, st.w16(b + "intermediate.dense.weight"), dc, n, W, I, I, W, W, b_tmaj=True, epilogue=ops.EPI_RESID_F32, resid=dt3)
    if not cx.cross:
        da = dc                      # mode "text": c32 is a32
    else:
        # ---- cross-attention sublayer: c = LN(co @ Wco^T + bco + a32)
        dt2 = ops.layernorm_bwd(sv["t2"], st.p(b + "crossattention.output.LayerNorm.weight"), dc,
                                G(b + "crossattention.output.LayerNorm.weight"), G(b + "crossattention.output.LayerNorm.bias"), eps,
                                dx_bf16=d16, rows=n, width=W)
        if ph:
            ops.dropout_bf16_(d16, ph, so2, row_map=rows.row_map)
        ops.linear_wgrad(d16, sv["co"], G(b + "crossattention.output.dense.weight"), dbias=G(b + "crossattention.output.dense.bias"))
        dco = ops.linear_dgrad(d16, st.w16(b + "crossattention.output.dense.weight"))
        dcq, dckv = cx.b16(n, W), cx.b16(cx.M * cx.Ti, 2 * W)
        rows.cross_bwd(sv, dco, dcq, dckv, sa2)
        img16 = cx.img16
        Ew = img16.shape[1]
        ops.linear_wgrad(dckv, img16, G(c + "key.weight", (2 * W, Ew)), dbias=G(c + "key.bias", (2 * W,)))
        ops.gemm(dckv, st.w16(c + "key.weight", (2 * W, Ew)), dimg, cx.M * cx.Ti, Ew, 2 * W, 2 * W, Ew, Ew, b_tmaj=True,
                 epilogue=ops.EPI_RESID_F32, resid=dimg)          # dimg += dckv @ Wkv (in place: same element r/w)
        ops.linear_wgrad(dcq, sv["a16"], G(c + "query.weight"), dbias=G(c + "query.bias"))
        da = cx.f32(n, W)       # d a32 = dcq @ Wcq + dt2
        ops.gemm(dcq, st.w16(c + "query.weight"), da, n, W, W, W, W, W, b_tmaj=True, epilogue=ops.EPI_RESID_F32, resid=dt2)
    # ---- self-attention sublayer: a = LN(ao @ Wo^T + bo + h32)
    dt1 = ops.layernorm_bwd(sv["t1"], st.p(b + "attention.output.LayerNorm.weight"), da, G(b + "attention.output.LayerNorm.weight"),
                            G(b + "attention.output.LayerNorm.bias"), eps, dx_bf16=d16, rows=n, width=W)
    if ph:
        ops.dropout_bf16_(d16, ph, so1, row_map=rows.row_map)
    ops.linear_wgrad(d16, sv["ao"], G(b + "attention.output.dense.weight"), dbias=G(b + "attention.output.dense.bias"))
    dao = ops.linear_dgrad(d16, st.w16(b + "attention.output.dense.weight"))
    dqkv = rows.self_bwd(sv, dao, sa1)          # on all R rows, whichever rows the layer ran on
    ops.linear_wgrad(dqkv, sv["h16"], G(s + "query.weight", (3 * W, W)), dbias=G(s + "query.bias", (3 * W,)))
    dh = cx.f32(cx.R, W)       # d h32 = dqkv @ Wqkv + dt1
    ops.gemm(dqkv, st.w16(s + "query.weight", (3 * W, W)), dh, cx.R, W, 3 * W, 3 * W, W, W, b_tmaj=True, epilogue=ops.EPI_RESID_F32,
             resid=rows.spread(dt1))
    return dh


def bert_forward(st, prefix, cfg, ids, key_len, img16, Ti, save, cross=True, pool=True, drop=None, pack=None, pool_last=False,
                 log=None, dtype16=torch.bfloat16):
    """src/models/uniir_blip/backbone/med.py BertModel.forward(mode="multimodal") -> pooler_output fp32 [M,W] + stash.
    ids int32 [M,L]; key_len int32 [M]; img16 bf16 [M*Ti, enc_width] (image attention mask all ones, blip_ff.py:98,108).
    cross=False: mode "text" (the cross-attention sublayer is skipped, BLIP_SF); pool=False: add_pooling_layer=False, the
    class-token row of last_hidden_state is returned instead of the tanh pooler output.
    drop (ops.DropSeeds, train mode): hidden dropout after the embedding LayerNorm and after each of the three output
    dense layers (before the residual add), attention-probability dropout inside both attention kernels.
    pack (TextPack): run on the rows up to each caption's valid length only -- same pooled output bit for bit (train mode included),
    parameter gradients equal up to the order of the fp32 additions in the weight-gradient reductions.
    pool_last (BLIPFeatureFusion.pool_last_layer): only the class row of every item leaves the encoder, so the LAST layer runs on
    those M rows (_ClassRows): the same class row bit for bit, train mode included.  log: a list that gets a line when it does.
    dtype16 = torch.float16 (forward only and eval only: save False, drop None; img16 fp16, or None for mode "text"): every weight
    comes from st's fp16 shadow (FlatStore.w16h, the spanning q | k | v and cross k | v shapes included), the 16-bit activations are
    fp16 and both attentions run the fp16 general form (ops.attention_fwd_ex_f16 / ops.onequery_fwd_f16); the residual stream, the
    LayerNorm statistics, tanh and the gathered class rows stay fp32, as in vit_forward.  pack and pool_last are honoured, each bit for
    bit the unpacked / full-layer result.  A bf16 caller makes exactly the calls it made before this argument existed."""
    M, L = ids.shape
    if dtype16 not in (torch.bfloat16, torch.float16):
        raise ValueError(f"dtype16 is torch.bfloat16 or torch.float16, not {dtype16!r}")
    half = dtype16 == torch.float16
    if half and (save or drop is not None):
        raise RuntimeError("the fp16 BERT forward is the eval-mode embedding forward: it keeps nothing for a backward and takes no "
                           "dropout (save=True and drop need dtype16=torch.bfloat16)")
    if half and img16 is not None and img16.dtype != torch.float16:
        raise ValueError(f"bert_forward: {img16.dtype} image tokens with dtype16 = {dtype16}")
    ph = cfg.get("hidden_dropout_prob", 0.0) if drop is not None else 0.0
    pa = cfg.get("attention_probs_dropout_prob", 0.0) if drop is not None else 0.0
    cx = _BertCall(st, prefix, cfg, M, L, Ti, key_len, img16, pack, ph, pa, cross, drop, dtype16)
    W, R, layers = cx.W, cx.R, cx.layers
    e32 = cx.f32(R, W)
    word, pos = st.p(prefix + "embeddings.word_embeddings.weight"), st.p(prefix + "embeddings.position_embeddings.weight")
    if pack is None:
        scratch = torch.empty(M, device=ids.device, dtype=torch.int32)
        ops.call("uniir_text_embed", ids, word, pos, e32, scratch, M, L, W, cx.vocab)
    else:
        ops.call("uniir_text_embed_packed", ids, word, pos, cx.roff, e32, None, M, L, W, cx.vocab)
    h32, h16 = cx.ln2(e32, prefix + "embeddings.LayerNorm.", R)
    s_emb = cx.seed(ph)
    if ph:
        ops.dropout_f32(h32, ph, s_emb, out_f32=h32, out_bf16=h16, row_map=cx.rmap)
    stash = dict(ids=ids, e32=e32, layers=[], M=M, L=L, Ti=Ti, key_len=key_len, img16=img16, ph=ph, pa=pa,
                 s_emb=s_emb, pack=pack) if save else None
    all_rows, class_rows = _AllRows(cx, layers - bool(pool_last)), _ClassRows(cx)
    for i in range(layers):
        rows = class_rows if pool_last and i == layers - 1 else all_rows
        h32, h16, sv = _layer_forward(cx, rows, i, h32, h16, save)
        if save:
            stash["layers"].append(sv)
    if pool_last:
        rows = h32
        if log is not None:
            log.append(f"BERT last layer {layers - 1} on the {M} class rows (pool_last_layer): K | V from {R} "
                       f"{'packed' if pack is not None else 'dense'} rows, {'self- and cross-' if cross else 'self-'}attention in the "
                       f"one-query form, {'stash of M-row tensors' if save else 'no stash'}")
    else:
        rows = class_rows.take(h32)          # the class token = the first row of every item
    if not pool:
        return rows, stash
    rows16 = cx.b16(M, W)
    ops.call("uniir_cast_f32_to_f16" if half else "uniir_cast_f32_to_bf16", rows, rows16, rows.numel())
    pre = ops.linear_fwd(rows16, cx.w16(prefix + "pooler.dense.weight"), st.p(prefix + "pooler.dense.bias"),
                         epilogue=ops.EPI_RESID_F32)
    pooled = torch.empty_like(pre)
    ops.call("uniir_tanh_fwd", pre, pooled, pre.numel())
    if save:
        stash.update(rows16=rows16, pooled=pooled)
    return pooled, stash


def bert_backward(st, prefix, cfg, dpooled, stash, cross=True, pool=True):
    """returns d(img tokens) fp32 [M*Ti, enc_width] (None without cross-attention); parameter gradients accumulate into
    st.g32.  dpooled: gradient of what bert_forward returned (pooler output, or the class-token rows with pool=False)"""
    cx = _BertCall.of_stash(st, prefix, cfg, stash, cross)
    G, M, L, W = st.grad_view, cx.M, cx.L, cx.W
    class_rows = _ClassRows(cx)
    do = _pooler_backward(cx, dpooled, stash) if pool else dpooled.contiguous().float()
    if not stash["layers"][-1].get("pooled"):          # else the last layer ran on the class rows and takes their gradient as it is
        do = class_rows.spread(do)
    dimg = cx.f32(M * cx.Ti, cx.img16.shape[1], zero=True) if cross else None
    all_rows = _AllRows(cx, sum(not sv.get("pooled") for sv in stash["layers"]))
    for i in reversed(range(cx.layers)):
        sv = stash["layers"][i]
        stash["layers"][i] = None
        do = _layer_backward(cx, class_rows if sv.get("pooled") else all_rows, i, sv, do, dimg)
    if cx.ph:
        ops.dropout_f32(do, cx.ph, stash["s_emb"], out_f32=do, row_map=cx.rmap)
    de = ops.layernorm_bwd(stash["e32"], st.p(prefix + "embeddings.LayerNorm.weight"), do,
                           G(prefix + "embeddings.LayerNorm.weight"), G(prefix + "embeddings.LayerNorm.bias"), cx.eps,
                           rows=cx.R, width=W)
    dword, dpos = G(prefix + "embeddings.word_embeddings.weight"), G(prefix + "embeddings.position_embeddings.weight")
    if cx.pack is None:
        ops.call("uniir_text_embed_bwd", stash["ids"], de, dword, dpos, M, L, W, cx.vocab)
    else:
        ops.call("uniir_text_embed_bwd_packed", stash["ids"], de, cx.roff, dword, dpos, M, L, W, cx.vocab)
    return dimg


def _pooler_backward(cx, dpooled, stash):
    """pooler: pooled = tanh(rows @ Wp^T + bp) -> the gradient of the class rows fp32 [M, W]"""
    st, G, M, W, name = cx.st, cx.st.grad_view, cx.M, cx.W, cx.prefix + "pooler.dense."
    dpre = cx.f32(M, W)
    ops.call("uniir_tanh_bwd", stash["pooled"], dpooled.contiguous(), dpre, dpre.numel())
    dpre16 = cx.b16(M, W)
    ops.call("uniir_cast_f32_to_bf16", dpre, dpre16, dpre.numel())
    ops.linear_wgrad(dpre16, stash["rows16"], G(name + "weight"))
    ops.call("uniir_colsum_bf16", dpre16, W, G(name + "bias"), M, W)
    drows = cx.f32(M, W)
    ops.gemm(dpre16, st.w16(name + "weight"), drows, M, W, W, W, W, W, b_tmaj=True, epilogue=ops.EPI_F32)
    return drows


# ------------------------------------------------------------------------------------------------------------
# fp32 forward (precision = "fp32"): the reference's model.float() embedding forward of BLIP's two encoders on the fp32 launch layer
# (fp32_forward.py), on the fp32 masters of the store: the ViT is its pre-LN tower, BERT's self-attention takes key_len and its
# cross-attention tq != tk.  It shares nothing with the dtype16 plumbing above.  Forward only; every row dense and every layer full.
# ------------------------------------------------------------------------------------------------------------
def vit_forward_f32(st, prefix, cfg, img_size, images):
    """vit_forward in fp32 -> fp32 tokens [M*T, D] after the final norm, and T"""
    p = lambda name: st.p(prefix + name)          # noqa: E731
    x, T = patch_tokens_f32(images, cfg["patch_size"], p("patch_embed.proj.weight"), p("patch_embed.proj.bias"), p("cls_token"),
                            p("pos_embed"))
    x = tower_fwd_f32(st.p, lambda i: _vit_blk_names(prefix, i), cfg["depth"], x, images.shape[0], T, cfg["embed_dim"],
                      cfg["num_heads"], False, eps=VIT_EPS, act=ops.ACT_GELU_ERF)
    return layernorm_f32(x, p("norm.weight"), p("norm.bias"), VIT_EPS), T


def bert_forward_f32(st, prefix, cfg, ids, key_len, img, Ti, cross=True, pool=True):
    """bert_forward in fp32 on the dense [M, L] rows -> fp32 [M, W]: the tanh pooler's output, or (pool=False) the class rows.
    img fp32 [M*Ti, enc_width] (None with cross=False, mode "text").  The padding mask is key_len: a padded key is skipped, which
    is the fp32 softmax the reference gets by adding -10000 to its logit (exp underflows to an exact 0)."""
    M, L = ids.shape
    W, eps, heads = cfg["hidden_size"], cfg["layer_norm_eps"], cfg["num_attention_heads"]
    dev = ids.device
    p = lambda name, shape=None: st.p(prefix + name, shape)          # noqa: E731

    def sublayer(x, name, resid):
        """dense + residual -> LayerNorm (BertSelfOutput / BertOutput)"""
        y = linear_f32(x, p(name + "dense.weight"), p(name + "dense.bias"), resid=resid)
        return layernorm_f32(y, p(name + "LayerNorm.weight"), p(name + "LayerNorm.bias"), eps)

    e = torch.empty(M * L, W, device=dev, dtype=torch.float32)
    scratch = torch.empty(M, device=dev, dtype=torch.int32)
    ops.call("uniir_text_embed", ids, p("embeddings.word_embeddings.weight"), p("embeddings.position_embeddings.weight"), e, scratch,
             M, L, W, cfg["vocab_size"])
    h = layernorm_f32(e, p("embeddings.LayerNorm.weight"), p("embeddings.LayerNorm.bias"), eps)
    for i in range(cfg["num_hidden_layers"]):
        b = f"encoder.layer.{i}."
        s, c = b + "attention.self.", b + "crossattention.self."
        qkv = linear_f32(h, p(s + "query.weight", (3 * W, W)), p(s + "query.bias", (3 * W,)))
        ao = attention_f32(qkv, 3 * W, qkv[:, W:], qkv[:, 2 * W:], 3 * W, key_len, M, L, L, heads)
        h = sublayer(ao, b + "attention.output.", h)
        if cross:
            cq = linear_f32(h, p(c + "query.weight"), p(c + "query.bias"))
            ckv = linear_f32(img, p(c + "key.weight", (2 * W, img.shape[1])), p(c + "key.bias", (2 * W,)))
            co = attention_f32(cq, W, ckv, ckv[:, W:], 2 * W, None, M, L, Ti, heads)
            h = sublayer(co, b + "crossattention.output.", h)
        f = linear_f32(h, p(b + "intermediate.dense.weight"), p(b + "intermediate.dense.bias"), act=ops.ACT_GELU_ERF)
        h = sublayer(f, b + "output.", h)
    rows = torch.empty(M, W, device=dev, dtype=torch.float32)
    ops.call("uniir_gather_rows", h, None, rows, M, L, W)          # the class token = row 0 of every item
    if not pool:
        return rows
    pre = linear_f32(rows, p("pooler.dense.weight"), p("pooler.dense.bias"))
    pooled = torch.empty_like(pre)
    ops.call("uniir_tanh_fwd", pre, pooled, pre.numel())
    return pooled


# ------------------------------------------------------------------------------------------------------------
# module
# ------------------------------------------------------------------------------------------------------------
class _EncodeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, ids, key_len, images, anchor, pack=None):
        save = bool(ctx.needs_input_grad[4])
        st = model._online
        drop = model._drop_seeds()
        tok, Ti, vst = vit_forward(st, "visual_encoder.", model.vit_cfg, model.image_size, images, save,
                                   drop=drop, recompute_from=model._vit_boundary(save))
        pooled, bst = bert_forward(st, "text_encoder.", model.med_cfg, ids, key_len, tok, Ti, save, drop=drop, pack=pack,
                                   pool_last=model.pool_last_layer, log=model._path_log())
        ctx.model, ctx.vst, ctx.bst = model, vst, bst
        return pooled

    @staticmethod
    def backward(ctx, dpooled):
        model, st = ctx.model, ctx.model._online
        bst, vst = ctx.bst, ctx.vst
        ctx.bst = ctx.vst = None
        dimg = bert_backward(st, "text_encoder.", model.med_cfg, dpooled, bst)
        vit_backward(st, "visual_encoder.", model.vit_cfg, dimg, vst)
        return None, None, None, None, None, None


class _SoftTargetLossFn(torch.autograd.Function):
    """blip_ff.py:155-231,250-252.  Everything that reads the queues runs in forward (the queues are overwritten before
    backward): the unit gradients are kept and scaled by d(loss) in backward.  With hard negatives (`ni` [b*N] rows of
    the flat batch, `ids_neg` their candidate ids) the candidate side is [p_m | nc_m (un-normalised, like the
    reference) | cand_queue[:, b*N:]] and the id row [p ids | negative ids | idx_queue[b*N:]] (:159-170,196-205)."""

    @staticmethod
    def forward(ctx, emb, temp, model, emb_m, qi, pi, ids_row, alpha, ni, ids_neg):
        b, E, dev = qi.numel(), emb.shape[1], emb.device
        K = model.queue_size
        n = b + K
        f32 = dict(device=dev, dtype=torch.float32)

        def sel(src, idx):
            rows = idx.numel()
            out, inv = torch.empty(rows, E, **f32), torch.empty(rows, **f32)
            ops.call("uniir_select_normalize", src, idx, out, inv, rows, E)
            return out, inv

        q, invq = sel(emb, qi)
        p, invp = sel(emb, pi)
        q_m, _ = sel(emb_m, qi)
        p_m, _ = sel(emb_m, pi)
        hn = 0
        nc_m = None
        if ni is not None:
            hn = ni.numel()
            nc_m = emb_m.index_select(0, ni.long()).contiguous()      # rows emb_m[ni], not normalised (a copy, no arithmetic)
            ids_all = torch.cat([ids_row, ids_neg, model.idx_queue[0, hn:]])
        else:
            ids_all = torch.cat([ids_row, model.idx_queue[0]])
        # column blocks of the two logit matrices: (row-major features [r,E]) or (queue [E,K], first column used)
        cand_blocks = [("rows", p_m, b)] + ([("rows", nc_m, hn)] if hn else []) + [("queue", model.cand_queue, hn)]
        query_blocks = [("rows", q_m, b), ("queue", model.query_queue, 0)]

        def sims(a, blocks):
            """[a @ block_0^T | a @ block_1^T | ...] without materialising the concatenation"""
            out = torch.empty(b, n, **f32)
            col = 0
            for kind, t, arg in blocks:
                if kind == "rows":
                    ops.call("uniir_sgemm", a, E, 1, t, 1, E, out[:, col:], n, b, arg, E, 1.0)
                    col += arg
                else:
                    ops.call("uniir_sgemm", a, E, 1, t[:, arg:], K, 1, out[:, col:], n, b, K - arg, E, 1.0)
                    col += K - arg
            return out

        def dfeat(dsim, blocks):
            """d a = sum over blocks of dsim[:, cols] @ block (the momentum / queue features carry no gradient)"""
            da = torch.empty(b, E, **f32)
            col, first = 0, True
            for kind, t, arg in blocks:
                fn = "uniir_sgemm" if first else "uniir_sgemm_acc"
                if kind == "rows":
                    ops.call(fn, dsim[:, col:], n, 1, t, E, 1, da, E, b, E, arg, 1.0)
                    col += arg
                else:       # reduction over the K queue columns, 2 x 6 output tiles: the deterministic split-K form
                    lib = _lib.load()
                    need_ws = int(lib.uniir_sgemm_splitk_workspace_bytes(b, E, K - arg))
                    ws = ops._splitk_workspace(da.device, need_ws, tag="blip_dfeat")
                    ops.call("uniir_sgemm_splitk", dsim[:, col:], n, 1, t[:, arg:], 1, K, da, E, b, E, K - arg, 1.0,
                             0 if first else 1, ws, ws.numel())
                    col += K - arg
                first = False
            return da

        need = ctx.needs_input_grad[0]
        rl, hit, rdt, dfe = [], None, [], []
        for a, a_m, blocks in ((q, q_m, cand_blocks), (p, p_m, query_blocks)):
            s, s_m = sims(a, blocks), sims(a_m, blocks)
            row_loss, row_hit = torch.empty(b, **f32), torch.empty(b, **f32)
            dsim = torch.empty(b, n, **f32) if need else None
            row_dt = torch.empty(b, **f32) if need else None
            ops.call("uniir_softce", s, s_m, temp, ids_row, ids_all, b, n, float(alpha), 1.0 / (2 * b), None, row_loss,
                     row_hit, dsim, row_dt)
            rl.append(row_loss)
            hit = row_hit if hit is None else hit
            if need:
                dfe.append(dfeat(dsim, blocks))
                rdt.append(row_dt)
        loss = (rl[0].sum() + rl[1].sum()) / (2 * b)
        acc = hit.mean()
        if need:
            demb = torch.zeros_like(emb)
            ops.call("uniir_select_normalize_bwd", q, invq, dfe[0], qi, demb, b, E)
            ops.call("uniir_select_normalize_bwd", p, invp, dfe[1], pi, demb, b, E)
            ctx.save_for_backward(demb, rdt[0].sum() + rdt[1].sum())
        if nc_m is None:
            nc_m = q_m.new_zeros(0, E)
        ctx.mark_non_differentiable(acc, q_m, p_m, nc_m)
        return loss, acc, q_m, p_m, nc_m

    @staticmethod
    def backward(ctx, dloss, _dacc, _dq, _dp, _dn):
        demb, dtemp = ctx.saved_tensors
        return demb * dloss, dtemp * dloss, None, None, None, None, None, None, None, None


class BLIPFeatureFusion(nn.Module):
    SCORE_FUSION = False

    def __init__(self, med_config="backbone/configs/med_config.json", image_size=224, vit="base", vit_grad_ckpt=False,
                 vit_ckpt_layer=0, embed_dim=768, queue_size=57600, momentum=0.995, config=None, seed=0,
                 vit_config=None):
        super().__init__()
        if isinstance(med_config, str):
            med_config = json.load(open(med_config))
        self.med_cfg = dict(MED_DEFAULT)
        self.med_cfg.update({k: v for k, v in dict(med_config).items() if k in MED_DEFAULT})
        self.vit_cfg = dict(vit_config or VIT_CONFIGS[vit])
        self.image_size = self.vit_cfg.get("img_size", image_size)
        W, D = self.med_cfg["hidden_size"], self.vit_cfg["embed_dim"]
        if W // self.med_cfg["num_attention_heads"] != 64 or D // self.vit_cfg["num_heads"] != 64 or W % 64 or D % 64:
            raise ValueError("the attention kernels are built for head_dim 64 (BLIP base / large both are)")
        sf = self.SCORE_FUSION
        if not sf and embed_dim != W:
            raise ValueError("BLIP_FF returns the BERT pooler output: embed_dim must equal the hidden size")
        self.med_cfg["encoder_width"] = D
        self.queue_size, self.momentum, self.embed_dim, self.config = queue_size, momentum, embed_dim, config
        vis = [("visual_encoder." + n, s) for n, s in vit_param_shapes(self.vit_cfg, self.image_size)]
        txt = [("text_encoder." + n, s) for n, s in bert_param_shapes(self.med_cfg, D, pooler=not sf)]
        if sf:     # blip_sf.py:35-47: no pooler, projection heads, cross-attention present but frozen -> kept at the END of
            # the flat stores so that the optimizer range stops before it (a frozen tensor must not see weight decay)
            proj = [("vision_proj.weight", (embed_dim, D)), ("vision_proj.bias", (embed_dim,)),
                    ("text_proj.weight", (embed_dim, W)), ("text_proj.bias", (embed_dim,))]
            self._frozen = {n for n, _ in txt if "crossattention" in n}
            self._shapes = vis + [t for t in txt if t[0] not in self._frozen] + proj + [t for t in txt if t[0] in self._frozen]
        else:
            self._frozen = set()
            self._shapes = vis + txt
        g = torch.Generator().manual_seed(seed)
        for n, shp in self._shapes:
            leaf = n.rsplit(".", 1)[-1]
            if "norm" in n.lower() and leaf == "weight":
                v = torch.ones(shp)
            elif leaf == "bias":
                v = torch.zeros(shp)
            else:
                v = torch.randn(shp, generator=g) * 0.02
            _attach(self, n, nn.Parameter(v, requires_grad=n not in self._frozen))
        for n, shp in self._shapes:      # momentum encoders start as copies (blip_ff.py:280-285 copy_params)
            enc, rest = n.split(".", 1)
            _attach(self, f"{enc}_m.{rest}", nn.Parameter(self.get_parameter(n).detach().clone(), requires_grad=False))
        self.text_encoder.embeddings.register_buffer(
            "position_ids", torch.arange(self.med_cfg["max_position_embeddings"]).expand((1, -1)))
        self.text_encoder_m.embeddings.register_buffer(
            "position_ids", torch.arange(self.med_cfg["max_position_embeddings"]).expand((1, -1)))
        self.register_buffer("query_queue", nn.functional.normalize(torch.randn(embed_dim, queue_size, generator=g), dim=0))
        self.register_buffer("cand_queue", nn.functional.normalize(torch.randn(embed_dim, queue_size, generator=g), dim=0))
        self.register_buffer("idx_queue", torch.full((1, queue_size), -100))
        self.register_buffer("new_ptr_queue", torch.zeros(1, dtype=torch.long))
        self.temp = nn.Parameter(0.07 * torch.ones([]))
        self._online = self._mom = None
        self._ptr_host = None
        self.check_masks = True
        # BERT on the rows up to each caption's valid length only (TextPack): same embeddings bit for bit, 47 % fewer BERT rows at
        # the bench's caption lengths.  False = the padded rows of the reference, all L positions (A/B, tests)
        self.pack_text = True
        self.last_text_rows = None        # (rows BERT ran on, M * L) of the last encode call (bench: executed FLOPs)
        # vit_grad_ckpt / vit_ckpt_layer (the reference's keys, large YAMLs: True / 12): the online ViT's blocks from this index on
        # keep only their fp32 input in a training forward and are rebuilt in the backward (vit_recompute_from); depth = every block
        # stored.  Bitwise the stored step's results, for one more pass over those blocks' sublayers.  A plain attribute: may be
        # changed between steps (A/B runs); must be the same on every rank.
        self.vit_recompute_from = vit_recompute_from(self.vit_cfg["depth"], vit_grad_ckpt, vit_ckpt_layer)
        self._vit_recompute_logged = False
        # Only the class row of every caption leaves the BERT (pooler_output / the class token), so its LAST layer needs the other
        # rows' keys and values only: with this on, that layer runs its attention in the one-query form and everything behind the
        # q | k | v projection on the M class rows (_bert_last_layer_pooled) -- online, momentum and no-grad passes, BLIP_SF too.
        # Embeddings, train-mode outputs and the loss are bitwise those of the full layer; weight gradients are the same sums over
        # fewer rows.  Off by default (profiles/blip_pooled_last_layer.txt has the measurement): UNIIR_BLIP_POOL_LAST_LAYER=1
        # switches it on at construction.  A plain attribute: may be changed between steps; must be the same on every rank.
        self.pool_last_layer = env_flag("UNIIR_BLIP_POOL_LAST_LAYER")
        # precision / embed_fp16 / embed_fp32: precision.py.  Here "fp16" and "fp32" are what encode_multimodal_input -- and with it
        # encode_mbeir_batch and forward(encode_mbeir_batch=True) -- runs: ViT and BERT (and BLIP_SF's projections), eval mode and the
        # online encoder only ("fp16" from the online store's fp16 shadow under a no_grad of its own, "fp32" under the caller's).  On
        # "fp32" pack_text, pool_last_layer and vit_grad_ckpt change nothing: every row is dense and every layer full (skipping padded
        # keys and adding -10000 to their logits are the same fp32 softmax).
        self.precision = "bf16"
        self.embed_fp16 = env_flag("UNIIR_BLIP_EMBED_FP16")
        self.embed_fp32 = env_flag("UNIIR_EMBED_FP32")
        self.path_log = []                # one line per BERT pass whose last layer ran on the class rows (the newest 64)

    def _path_log(self):
        """the list bert_forward reports to when pool_last_layer is on (trimmed here: it grows by one line per encoder pass)"""
        del self.path_log[:-63]
        return self.path_log

    def _vit_boundary(self, save):
        """recompute_from of a ViT forward of the online encoder; the first training forward that recomputes says so once"""
        depth, k = self.vit_cfg["depth"], self.vit_recompute_from
        if save and k < depth and not self._vit_recompute_logged:
            self._vit_recompute_logged = True
            logging.getLogger(__name__).info(
                "BLIP ViT: blocks %d..%d of %d are recomputed in the backward (vit_grad_ckpt / vit_ckpt_layer): only their inputs "
                "are kept; results are bitwise those of the stored step. vit_grad_ckpt: False keeps the whole stash.",
                max(k, 0), depth - 1, depth)
        return k

    # ---- reference surface ---------------------------------------------------------------------------------
    def get_img_preprocess_fn(self, raw=False, randaugment=None):
        """raw=True: the deferred form of the same transform (blip_front.RawBlipTransform) -- the workers decode and draw the
        crop box / flip, the batched device transform does the rest; also set it as the collator's `raw_transform`.
        randaugment=(N, M): the reference's RandomAugment(N, M) in train mode (upstream trains with (2, 5)); either form"""
        from .blip_front import RawBlipTransform, get_blip_transform
        if raw:
            return RawBlipTransform(self.image_size, min_scale=0.5, is_train=self.training, randaugment=randaugment)
        return get_blip_transform(self.image_size, min_scale=0.5, is_train=self.training, randaugment=randaugment)

    def get_tokenizer(self):
        from .blip_front import init_tokenizer
        tok = init_tokenizer()
        max_len = self.config.tokenizer_max_length

        def tokenizer_wrapper(txt):
            return tok(txt, padding="max_length", truncation=True, max_length=max_len, return_tensors="pt")

        return tokenizer_wrapper

    @torch.no_grad()
    def copy_params(self):
        for n, pm in self._momentum_params():
            pm.data.copy_(self.get_parameter(n).data)

    # ---- flat storage --------------------------------------------------------------------------------------
    def _online_params(self):
        return [(n, self.get_parameter(n)) for n, _ in self._shapes] + [("temp", self.temp)]

    def _momentum_params(self):
        """the momentum encoders' parameters under the ONLINE names: both stores have one layout and one launch sequence"""
        return [(n, self.get_parameter("{}_m.{}".format(*n.split(".", 1)))) for n, _ in self._shapes]

    def _ensure_flat(self):
        dev = self.temp.device
        if dev.type != "cuda":
            raise RuntimeError("uniir_amd BLIPFeatureFusion runs on an MI355X only (no CPU path); move the model to cuda")
        if self._online is not None and self._online.holds(self._online_params()):
            return self._online
        # temp has no shadow and is clamp_()ed every step: its version is not watched
        self._online = FlatStore.adopt(self._online_params(), dev, frozen=self._frozen, unversioned=("temp",))
        self._mom = FlatStore.adopt(self._momentum_params(), dev, with_grad=False)
        D, P = self.vit_cfg["embed_dim"], self.vit_cfg["patch_size"]
        for st in (self._online, self._mom):
            st.add_padded("visual_encoder." + CONV, D, 3 * P * P, patch_kpad(P))
        self.refresh_shadow()
        return self._online

    def optimizer_groups(self):
        """(no-decay params, decay params) for NativeAdamW: the reference applies weight decay to every parameter
        (uniir_blip/train.py:193-197)"""
        return [], [p for n, p in self._online_params() if n not in self._frozen]

    def adamw_group(self, name):
        """NativeAdamW's param group of tensor `name`: the weight-decay group; frozen tensors (BLIP_SF's cross-attention, between
        the trainable tensors and temp) are not stepped"""
        return None if name in self._frozen else 1

    def refresh_shadow(self):
        self._online.refresh_shadow()
        self._mom.refresh_shadow()

    def _sync(self, half=False):
        """both stores, their bf16 copies following torch-side writes (FlatStore.sync); half: the online store's fp16 copies too"""
        self._ensure_flat()
        self._online.sync()
        self._mom.sync()
        if half:
            self._online.half_shadow()

    def zero_grad(self, set_to_none=False):
        if self._online is not None:
            self._online.zero_grad(self._online_params(), self._frozen)
        else:
            super().zero_grad(set_to_none=set_to_none)

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._ptr_host = None
        return out

    # ---- encoders ------------------------------------------------------------------------------------------
    def _drop_seeds(self):
        """train mode with a non-zero rate: a fresh seed stream for one encoder pass (else None: no dropout launches)"""
        rates = (self.med_cfg.get("hidden_dropout_prob", 0.0), self.med_cfg.get("attention_probs_dropout_prob", 0.0),
                 self.vit_cfg.get("drop_path_rate", 0.0))
        return ops.DropSeeds() if self.training and any(r > 0 for r in rates) else None

    def _text_inputs(self, txt):
        ids = txt["input_ids"] if isinstance(txt, dict) else txt.input_ids
        mask = txt["attention_mask"] if isinstance(txt, dict) else txt.attention_mask
        if self.check_masks and not bool((mask[:, :-1] >= mask[:, 1:]).all()):
            raise ValueError("attention_mask must be a prefix mask (ones, then padding): tokenizer padding='max_length'")
        return ids.to(torch.int32).contiguous(), mask.sum(1).to(torch.int32).contiguous()

    def _text_pack(self, txt, key_len, L):
        """the TextPack of this token batch (None: pack_text off, or nothing to drop).  Built once per batch -- the online and the
        momentum encoder of a step see the same tokens -- and remembered on the attention-mask tensor under its version."""
        if not self.pack_text:
            return None
        mask = txt["attention_mask"] if isinstance(txt, dict) else txt.attention_mask
        try:
            ver = mask._version
        except RuntimeError:
            ver = None
        hit = getattr(mask, "_uniir_pack", None)
        if ver is not None and hit is not None and hit[0] == ver and hit[1] == L:
            return hit[2]
        # the captions' lengths on the host: attached by the prefetcher while the mask was still there (mask._uniir_lens, tied to the
        # tensor version like CLIP's hint), else one device -> host read
        lens = getattr(mask, "_uniir_lens", None)
        if (isinstance(lens, torch.Tensor) and not lens.is_cuda and lens.dim() == 1 and lens.shape[0] == mask.shape[0]
                and not lens.is_floating_point() and ver is not None and getattr(mask, "_uniir_lens_version", None) == ver):
            pack = TextPack.build(lens, L, key_len.device)
        else:
            pack = TextPack.build(key_len, L)
        if ver is not None:
            mask._uniir_pack = (ver, L, pack)
        return pack

    @torch.no_grad()
    def _vit_tokens(self, image_batched, precision="bf16"):
        """Internal (the ViT leg of an fp16 embedding forward, and what the tests and tools/blip_vit_rate.py drive; not part of the
        model's surface).  The online vision encoder on its own, forward only (no stash, no graph): the normed tokens [n, T, D] in
        the 16-bit type of `precision`.  "bf16": the kernels of the training forward.  "fp16": the same launch sequence on fp16 operands and
        activations from fp16 copies of the weights (vit_forward's dtype16) -- the reference embedder's arithmetic
        (mbeir_embedder.py:52-56: autocast(fp16)), 577 tokens at 384 pixels included.  fp16 is an eval-mode path: in training mode
        it raises (DropPath belongs to the bf16 training forward)."""
        check_mode(precision, ("bf16", "fp16"), self.training)
        half = precision == "fp16"
        self._sync(half)
        tok, T, _ = vit_forward(self._online, "visual_encoder.", self.vit_cfg, self.image_size, image_batched, False,
                                drop=None if half else self._drop_seeds(), dtype16=torch.float16 if half else torch.bfloat16)
        return tok.view(image_batched.shape[0], T, -1)

    def _embed_mode(self, use_momentum):
        return embed_mode(self, use_momentum=use_momentum)

    def _encode_inputs(self, txt_dict_batched, use_momentum):
        """what every encode call starts with: the stores brought up to date, the token ids and key lengths, the TextPack
        -> mode (_embed_mode), ids, key_len, pack; last_text_rows = (BERT rows run, rows of the padded batch).  "fp32" runs the dense
        rows: no pack"""
        mode = self._embed_mode(use_momentum)
        self._sync(half=mode == "fp16")
        ids, key_len = self._text_inputs(txt_dict_batched)
        pack = self._text_pack(txt_dict_batched, key_len, ids.shape[1]) if mode != "fp32" else None
        self.last_text_rows = (pack.R if pack is not None else ids.numel(), ids.numel())
        return mode, ids, key_len, pack

    def encode_multimodal_input(self, txt_dict_batched, image_batched, txt_mask=None, img_mask=None, use_momentum=False):
        """blip_ff.py:82-116: BERT(text) cross-attending to ViT(image) tokens -> pooler_output [n, embed_dim]"""
        mode, ids, key_len, pack = self._encode_inputs(txt_dict_batched, use_momentum)
        if mode == "fp32":
            st = self._online
            tok, Ti = vit_forward_f32(st, "visual_encoder.", self.vit_cfg, self.image_size, image_batched)
            return bert_forward_f32(st, "text_encoder.", self.med_cfg, ids, key_len, tok, Ti)
        if mode == "fp16":
            with torch.no_grad():
                st = self._online
                tok, Ti, _ = vit_forward(st, "visual_encoder.", self.vit_cfg, self.image_size, image_batched, False,
                                         dtype16=torch.float16)
                return bert_forward(st, "text_encoder.", self.med_cfg, ids, key_len, tok, Ti, False, pack=pack,
                                    pool_last=self.pool_last_layer, log=self._path_log(), dtype16=torch.float16)[0]
        if use_momentum:
            with torch.no_grad():
                drop = self._drop_seeds()
                tok, Ti, _ = vit_forward(self._mom, "visual_encoder.", self.vit_cfg, self.image_size, image_batched, False,
                                         drop=drop)
                return bert_forward(self._mom, "text_encoder.", self.med_cfg, ids, key_len, tok, Ti, False, drop=drop,
                                    pack=pack, pool_last=self.pool_last_layer, log=self._path_log())[0]
        anchor = torch.zeros(1, device=ids.device, requires_grad=torch.is_grad_enabled())
        return _EncodeFn.apply(self, ids, key_len, image_batched, anchor, pack)

    @torch.no_grad()
    def _momentum_update(self):
        """blip_ff.py:287-292 as one fused pass over the flat encoder region (temp sits after it)"""
        self._sync()
        ops.call("uniir_ema_update", self._mom.p32, self._online.p32, self._mom.w16_buf, self._mom.total,
                 float(self.momentum))
        self._mom.kernel_wrote()

    @torch.no_grad()
    def _dequeue_and_enqueue(self, query_feats, cand_feats, idxs):
        """blip_ff.py:294-310"""
        idxs = comm.all_gather_rows(idxs.view(-1, 1))
        query_feats = comm.all_gather_rows(query_feats)
        cand_feats = comm.all_gather_rows(cand_feats)
        bsz = query_feats.shape[0]
        if self._ptr_host is None:
            self._ptr_host = int(self.new_ptr_queue)
        ptr = self._ptr_host
        assert self.queue_size % bsz == 0  # same requirement as the reference
        self.query_queue[:, ptr:ptr + bsz] = query_feats.T
        self.cand_queue[:, ptr:ptr + bsz] = cand_feats.T
        self.idx_queue[:, ptr:ptr + bsz] = idxs.T
        self._ptr_host = (ptr + bsz) % self.queue_size
        self.new_ptr_queue.fill_(self._ptr_host)

    def compute_contrastive_loss(self, batch, alpha):
        index_mapping = batch["index_mapping"]
        hard = "neg_cand_list" in index_mapping
        dev = self.temp.device
        txt, img = batch["txt_batched"], batch["image_batched"]
        ids_row = torch.as_tensor(batch["p_did_list"], device=dev).to(torch.int64).flatten()
        qi = torch.tensor(index_mapping["query"], dtype=torch.int32).flatten().to(dev)
        pi = torch.tensor(index_mapping["pos_cand"], dtype=torch.int32).flatten().to(dev)
        ni = ids_neg = None
        if hard:     # blip_ff.py:127-131: [bs, neg_num] rows of the flat batch and their candidate ids
            ni = torch.tensor(index_mapping["neg_cand_list"], dtype=torch.int32).flatten().to(dev)
            ids_neg = torch.as_tensor(batch["nc_dids_list"], device=dev).to(torch.int64).flatten()
        with torch.no_grad():
            self.temp.clamp_(0.001, 0.5)
        emb = self.encode_multimodal_input(txt, img, batch.get("txt_mask_batched"), batch.get("image_mask_batched"))
        self._momentum_update()
        emb_m = self.encode_multimodal_input(txt, img, batch.get("txt_mask_batched"), batch.get("image_mask_batched"),
                                             use_momentum=True)
        loss, acc, q_m, p_m, nc_m = _SoftTargetLossFn.apply(emb, self.temp, self, emb_m, qi, pi, ids_row, alpha, ni, ids_neg)
        if hard and not bool(torch.rand(1) < 0.5):
            # blip_ff.py:233-246: a coin flip (same host generator as the reference) enqueues each query's FIRST negative
            bs = qi.numel()
            nneg = ni.numel() // bs
            self._dequeue_and_enqueue(q_m.detach(), nc_m.detach().view(bs, nneg, -1)[:, 0, :].contiguous(),
                                      ids_neg.view(bs, nneg)[:, 0].contiguous())
        else:
            self._dequeue_and_enqueue(q_m.detach(), p_m.detach(), ids_row)
        return {"loss": loss, "accuracy": acc}

    def encode_mbeir_batch(self, batch):
        id_list = batch.get("did_list") or batch.get("qid_list")
        if id_list is None:
            raise ValueError("id_list not found in batch.")
        emb = self.encode_multimodal_input(batch["txt_batched"], batch["image_batched"], batch.get("txt_mask_batched"),
                                           batch.get("image_mask_batched"))
        assert emb.size(0) == len(id_list), "embeddings and id_batched must have the same batch size."
        return emb, id_list

    def forward(self, batch, alpha=None, encode_mbeir_batch=False):
        if encode_mbeir_batch:
            return self.encode_mbeir_batch(batch)
        return self.compute_contrastive_loss(batch, alpha)


class _EncodeSFFn(torch.autograd.Function):
    """BLIP_SF encoder (blip_sf.py:97-172): text_proj(BERT mode "text" class token) * txt_mask + vision_proj(ViT class
    token) * img_mask"""

    @staticmethod
    def forward(ctx, model, ids, key_len, images, tmask, imask, anchor, pack=None):
        save = bool(ctx.needs_input_grad[6])
        emb, stash = model._encode_sf(model._online, ids, key_len, images, tmask, imask, save, pack)
        ctx.model, ctx.stash = model, stash
        return emb

    @staticmethod
    def backward(ctx, demb):
        model, st, S = ctx.model, ctx.model._online, ctx.stash
        ctx.stash = None
        M, E = demb.shape
        dev = demb.device
        G = st.grad_view
        dt, di = torch.empty(M, E, device=dev), torch.empty(M, E, device=dev)
        ops.call("uniir_fuse_embeddings_bwd", demb.contiguous(), S["tmask"], S["imask"], dt, di, M, E)

        def proj_bwd(dy, x16, name):
            dy16 = torch.empty(M, E, device=dev, dtype=torch.bfloat16)
            ops.call("uniir_cast_f32_to_bf16", dy, dy16, dy.numel())
            ops.linear_wgrad(dy16, x16, G(name + ".weight"), dbias=G(name + ".bias"))
            K = x16.shape[1]
            dx = torch.empty(M, K, device=dev, dtype=torch.float32)
            ops.gemm(dy16, st.w16(name + ".weight"), dx, M, K, E, E, K, K, b_tmaj=True, epilogue=ops.EPI_F32)
            return dx

        dtfeat = proj_bwd(dt, S["tfeat16"], "text_proj")
        difeat = proj_bwd(di, S["ifeat16"], "vision_proj")
        bert_backward(st, "text_encoder.", model.med_cfg, dtfeat, S["bst"], cross=False, pool=False)
        T, D = S["T"], difeat.shape[1]
        dtok = torch.zeros(M * T, D, device=dev, dtype=torch.float32)
        ops.call("uniir_scatter_rows", difeat, None, dtok, M, T, D)
        vit_backward(st, "visual_encoder.", model.vit_cfg, dtok, S["vst"])
        return None, None, None, None, None, None, None, None


class BLIPScoreFusion(BLIPFeatureFusion):
    """src/models/uniir_blip/blip_scorefusion/blip_sf.py: the same momentum / queue loss as BLIP_FF on score-fused
    embeddings; state-dict keys add vision_proj{,_m}.* / text_proj{,_m}.*, the BERT has no pooler, its cross-attention
    parameters exist but are frozen (:66-69) and unused (mode "text")."""
    SCORE_FUSION = True

    def _encode_sf(self, st, ids, key_len, images, tmask, imask, save, pack=None, dtype16=torch.bfloat16):
        """dtype16 = torch.float16 (the fp16 embedding forward: save False, eval mode): ViT, BERT and the two projections on fp16
        operands from st's fp16 shadow"""
        dev = ids.device
        M = ids.shape[0]
        E = self.embed_dim
        half = dtype16 == torch.float16
        w16 = st.w16h if half else st.w16
        drop = None if half else self._drop_seeds()
        tok, T, vst = vit_forward(st, "visual_encoder.", self.vit_cfg, self.image_size, images, save, drop=drop,
                                  recompute_from=self._vit_boundary(save), dtype16=dtype16)
        ifeat16 = tok.view(M, T, -1)[:, 0].contiguous()                     # class-token rows (a copy)
        tfeat, bst = bert_forward(st, "text_encoder.", self.med_cfg, ids, key_len, None, 0, save, cross=False, pool=False,
                                  drop=drop, pack=pack, pool_last=self.pool_last_layer, log=self._path_log(), dtype16=dtype16)
        tfeat16 = torch.empty(M, tfeat.shape[1], device=dev, dtype=dtype16)
        ops.call("uniir_cast_f32_to_f16" if half else "uniir_cast_f32_to_bf16", tfeat, tfeat16, tfeat.numel())
        temb = ops.linear_fwd(tfeat16, w16("text_proj.weight"), st.p("text_proj.bias"), epilogue=ops.EPI_RESID_F32)
        iemb = ops.linear_fwd(ifeat16, w16("vision_proj.weight"), st.p("vision_proj.bias"), epilogue=ops.EPI_RESID_F32)
        emb = torch.empty(M, E, device=dev, dtype=torch.float32)
        ops.call("uniir_fuse_embeddings", temb, iemb, tmask, imask, emb, M, E)
        stash = dict(vst=vst, bst=bst, T=T, tfeat16=tfeat16, ifeat16=ifeat16, tmask=tmask, imask=imask) if save else None
        return emb, stash

    def _encode_sf_f32(self, st, ids, key_len, images, tmask, imask):
        """_encode_sf in fp32 (precision = "fp32"): vit_forward_f32 / bert_forward_f32 in mode "text", the two projections by
        uniir_sgemm, the mask fusion as the bf16 path does it"""
        M, E = ids.shape[0], self.embed_dim
        tok, T = vit_forward_f32(st, "visual_encoder.", self.vit_cfg, self.image_size, images)
        ifeat = tok.view(M, T, -1)[:, 0].contiguous()                     # class-token rows (a copy)
        tfeat = bert_forward_f32(st, "text_encoder.", self.med_cfg, ids, key_len, None, 0, cross=False, pool=False)
        temb = linear_f32(tfeat, st.p("text_proj.weight"), st.p("text_proj.bias"))
        iemb = linear_f32(ifeat, st.p("vision_proj.weight"), st.p("vision_proj.bias"))
        emb = torch.empty(M, E, device=ids.device, dtype=torch.float32)
        ops.call("uniir_fuse_embeddings", temb, iemb, tmask, imask, emb, M, E)
        return emb

    def encode_multimodal_input(self, txt_dict_batched, image_batched, txt_mask=None, img_mask=None, use_momentum=False):
        mode, ids, key_len, pack = self._encode_inputs(txt_dict_batched, use_momentum)
        M = ids.shape[0]
        dev = ids.device
        ones = torch.ones(M, dtype=torch.int64, device=dev)
        tmask = ones if txt_mask is None else txt_mask.to(dev).to(torch.int64).contiguous()
        imask = ones if img_mask is None else img_mask.to(dev).to(torch.int64).contiguous()
        if mode == "fp32":
            return self._encode_sf_f32(self._online, ids, key_len, image_batched, tmask, imask)
        if mode == "fp16":
            with torch.no_grad():
                return self._encode_sf(self._online, ids, key_len, image_batched, tmask, imask, False, pack, torch.float16)[0]
        if use_momentum:
            with torch.no_grad():
                return self._encode_sf(self._mom, ids, key_len, image_batched, tmask, imask, False, pack)[0]
        anchor = torch.zeros(1, device=dev, requires_grad=torch.is_grad_enabled())
        return _EncodeSFFn.apply(self, ids, key_len, image_batched, tmask, imask, anchor, pack)


def blip_sf(pretrained="", **kwargs):
    model = BLIPScoreFusion(**kwargs)
    if pretrained:
        from .host_utils import load_checkpoint_file
        sd = load_checkpoint_file(pretrained)
        msg = model.load_state_dict(sd.get("model", sd), strict=False)
        print("missing keys:")
        print(msg.missing_keys)
    return model


def blip_ff(pretrained="", **kwargs):
    model = BLIPFeatureFusion(**kwargs)
    if pretrained:
        from .host_utils import load_checkpoint_file
        sd = load_checkpoint_file(pretrained)
        msg = model.load_state_dict(sd.get("model", sd), strict=False)
        print("missing keys:")
        print(msg.missing_keys)
    return model
