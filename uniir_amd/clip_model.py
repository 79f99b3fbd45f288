"""MI355X-native CLIP towers behind the openai/CLIP module surface that UniIR's clip_sf.py uses
(`clip.load()` -> model with .encode_image / .encode_text / .logit_scale, state-dict keys of the published
checkpoints: SURVEY.md section 3.2; reference call sites src/models/uniir_clip/clip_scorefusion/clip_sf.py:25-26,
44,47,66).

The arithmetic is entirely in libuniir_hip.so (include/uniir_hip.h): bf16 MFMA GEMMs with fused epilogues,
fp32 LayerNorm, fused attention, fp32 residual stream.  This file is host plumbing only: parameter bookkeeping
(flat_store.FlatStore: one flat fp32 master buffer + flat grad buffer + bf16 shadow), the calls of the C towers
(csrc/tower.hip), the fp32 forward's launch sequence and the activation stash.  There is no torch fallback.
"""
import contextlib
import ctypes as C
import math
import os

import torch
from torch import nn

from . import _lib, ops
from .flat_store import FlatStore, patch_kpad
from .fp32_forward import layernorm_f32, linear_f32, patch_tokens_f32, tower_fwd_f32
from .precision import env_flag
from .resblocks import clip_block_names

CONV = "visual.conv1.weight"          # the patch-embedding weight: the store keeps its [width, kpad] copies (FlatStore.add_padded)
_SIDE_STREAMS = {}          # device index -> the torch stream that carries the text leg of two-stream towers (CLIP.side_leg)

def _tensor_version(t):
    try:
        return t._version
    except RuntimeError:            # inference tensors (torch.inference_mode) have no version counter: never cache on them
        return None


def text_row_offsets(tok):
    """(row_off int32 [n + 1] on the tokens' device, live rows on the host) of a token batch [n, ctx]: caption i owns
    argmax(tok[i]) + 1 rows (upstream pools at the EOT = the largest token id, first occurrence).  The host needs the total to size
    the GEMMs, which costs one device -> host read per NEW batch; a prefetcher that still has the tokens on the host can attach
    the lengths as `tok._uniir_lens` (+ `tok._uniir_lens_version`; host_utils.DevicePrefetcher does).  The hint is used only if it is
    a host tensor of n lengths in [1, ctx] attached to THIS version of the tensor -- anything else (tokens modified in place after the
    prefetch, a foreign attribute) falls back to the device read, so a stale hint can never size or index the packed kernels.  The
    result is remembered ON the tensor object (with its version counter), so a batch that is fed repeatedly (benchmarks, gradient
    accumulation replays) pays the read once; nothing is keyed by address, so a recycled allocation can never produce a stale answer."""
    ver = _tensor_version(tok)
    hit = getattr(tok, "_uniir_row_off", None)
    if hit is not None and ver is not None and hit[0] == ver and hit[1] == tuple(tok.shape):
        return hit[2]
    n, ctx = tok.shape
    lens = getattr(tok, "_uniir_lens", None)
    if lens is not None:
        ok = (isinstance(lens, torch.Tensor) and not lens.is_cuda and lens.dim() == 1 and lens.shape[0] == n
              and not lens.is_floating_point() and getattr(tok, "_uniir_lens_version", ver) == ver)
        if ok:
            lens = lens.to(torch.int64)
            ok = n == 0 or bool(((lens >= 1) & (lens <= ctx)).all())
        if not ok:
            lens = None
    if lens is None:
        lens = (tok.argmax(dim=-1) + 1).to(torch.int64).cpu()          # always in [1, ctx]
    off = torch.zeros(n + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(lens, 0)
    out = (off.to(torch.int32).to(tok.device), int(off[-1]))
    if ver is not None:
        try:
            tok._uniir_row_off = (ver, tuple(tok.shape), out)
        except Exception:
            pass
    return out

CLIP_CONFIGS = {
    "ViT-B/32": dict(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32,
                     context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8,
                     transformer_layers=12),
    "ViT-B/16": dict(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=16,
                     context_length=77, vocab_size=49408, transformer_width=512, transformer_heads=8,
                     transformer_layers=12),
    "ViT-L/14": dict(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14,
                     context_length=77, vocab_size=49408, transformer_width=768, transformer_heads=12,
                     transformer_layers=12),
    # ViT-L/14 at 336 pixels: 24 x 24 + 1 = 577 tokens (the vision tower's attention streams K / V, csrc/attention_long.hip)
    "ViT-L/14@336px": dict(embed_dim=768, image_resolution=336, vision_layers=24, vision_width=1024, vision_patch_size=14,
                           context_length=77, vocab_size=49408, transformer_width=768, transformer_heads=12,
                           transformer_layers=12),
}


def _is_no_decay(name, p):
    # UniIR clip_scorefusion/train.py:195: p.ndim < 2 or name contains bn / ln / bias / logit_scale
    return p.ndim < 2 or any(s in name for s in ["bn", "ln", "bias", "logit_scale"])


class _P(nn.Module):
    """bare parameter holder so that state-dict keys match upstream module paths"""

    def __init__(self, **params):
        super().__init__()
        for k, v in params.items():
            self.register_parameter(k, nn.Parameter(v))


def _resblocks(width, layers, gen):
    proj_std = (width ** -0.5) * ((2 * layers) ** -0.5)
    attn_std = width ** -0.5
    fc_std = (2 * width) ** -0.5

    def rn(*shape, std):
        return torch.randn(*shape, generator=gen) * std

    blocks = nn.ModuleList()
    for _ in range(layers):
        blk = nn.Module()
        blk.attn = _P(in_proj_weight=rn(3 * width, width, std=attn_std), in_proj_bias=torch.zeros(3 * width))
        blk.attn.out_proj = _P(weight=rn(width, width, std=proj_std), bias=torch.zeros(width))
        blk.ln_1 = _P(weight=torch.ones(width), bias=torch.zeros(width))
        blk.mlp = nn.Module()
        blk.mlp.c_fc = _P(weight=rn(4 * width, width, std=fc_std), bias=torch.zeros(4 * width))
        blk.mlp.c_proj = _P(weight=rn(width, 4 * width, std=proj_std), bias=torch.zeros(width))
        blk.ln_2 = _P(weight=torch.ones(width), bias=torch.zeros(width))
        blocks.append(blk)
    t = nn.Module()
    t.resblocks = blocks
    return t


class CLIP(nn.Module):
    """Same attribute / key layout as upstream clip.model.CLIP (visual.*, transformer.*, token_embedding.weight, ...)."""

    def __init__(self, cfg, seed=0):
        super().__init__()
        self.cfg = dict(cfg)
        g = torch.Generator().manual_seed(seed)
        vw, tw, E, P = cfg["vision_width"], cfg["transformer_width"], cfg["embed_dim"], cfg["vision_patch_size"]
        grid = cfg["image_resolution"] // P
        scale = vw ** -0.5
        self.visual = nn.Module()
        self.visual.conv1 = _P(weight=torch.randn(vw, 3, P, P, generator=g) * (1.0 / (3 * P * P)) ** 0.5)
        self.visual.register_parameter("class_embedding", nn.Parameter(torch.randn(vw, generator=g) * scale))
        self.visual.register_parameter("positional_embedding",
                                       nn.Parameter(torch.randn(grid * grid + 1, vw, generator=g) * scale))
        self.visual.ln_pre = _P(weight=torch.ones(vw), bias=torch.zeros(vw))
        self.visual.transformer = _resblocks(vw, cfg["vision_layers"], g)
        self.visual.ln_post = _P(weight=torch.ones(vw), bias=torch.zeros(vw))
        self.visual.register_parameter("proj", nn.Parameter(torch.randn(vw, E, generator=g) * scale))
        self.transformer = _resblocks(tw, cfg["transformer_layers"], g)
        self.token_embedding = _P(weight=torch.randn(cfg["vocab_size"], tw, generator=g) * 0.02)
        self.positional_embedding = nn.Parameter(torch.randn(cfg["context_length"], tw, generator=g) * 0.01)
        self.ln_final = _P(weight=torch.ones(tw), bias=torch.zeros(tw))
        self.text_projection = nn.Parameter(torch.randn(tw, E, generator=g) * tw ** -0.5)
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        self._flat = None          # the FlatStore of the parameters (built lazily on the device, _ensure_flat)
        self.kpad = patch_kpad(P)
        # precision / embed_fp32: precision.py.  Here "fp16" and "fp32" are the C towers' forward-only paths (_TowerFn); the weights of
        # "fp16" are read from an fp16 shadow that is refreshed with the bf16 one.
        self.precision = "bf16"
        self.embed_fp32 = env_flag("UNIIR_EMBED_FP32")
        # exact text-row packing (csrc/tower.hip *_packed): the text tower runs on the tokens up to each caption's EOT only.  Rows
        # behind the EOT never reach the pooled feature under the causal mask (clip_sf.py:43-44), so results are those of the dense
        # tower (embeddings and activation gradients bitwise, weight gradients up to the order of fp32 additions).
        self.pack_text = True
        # act(f) of every MLP kept per layer by the forward (uniir_clip_tower.stash_act) instead of being re-materialised by the c_proj
        # dgrad epilogue: +2 B x rows x 4 width per layer of workspace (52 GB at ViT-L/14 x 1024 items), bitwise the same results.
        # None = automatic, True / False = forced.  Automatic: decided ONCE per tower -- at the first training forward, from
        # the device's free memory with stash_margin_bytes to spare -- and then kept (the choice moves weight-gradient bits by fp32
        # summation order, so a run must not flip it from step to step or differ between ranks: see review_stash for W > 1);
        # an out-of-memory error on the stash allocation re-plans that tower without it; review_stash() revisits the choice after the
        # first complete step, when collectives' buffers and the optimizer state exist.
        self.stash_act = None
        # The last residual block of a POOLING tower on the pooled rows only (uniir_clip_tower.pool_last_block, csrc/tower.hip): the
        # class token / the EOT row is all that leaves the tower (clip_sf.py:44,47 -> upstream ln_post(x[:, 0, :]) /
        # x[arange, text.argmax(-1)]), so in the last block only ln_1 and the K | V projection need every row.  Exact: the same
        # embedding, the same parameter gradients without their zero terms.  False = every row through every sublayer (A/B, tests).
        self.pool_last_block = os.environ.get("UNIIR_POOL_LAST_BLOCK", "1") != "0"
        # ... above 512 tokens too (uniir_clip_tower.pool_last_block = 2; ViT-L/14@336px: 577 tokens): the block's one-query attention
        # then runs the streaming forward at one query row and the one-pass backward of csrc/attention_one.hip.  Same embeddings bit for
        # bit; the gradients upstream of the last block's attention agree with the full block's to bf16 rounding (another valid bf16
        # backward kernel), so it is off by default: UNIIR_POOL_LAST_BLOCK_LONG=1 switches it on at construction.  Without
        # pool_last_block it does nothing; at 512 tokens and below it changes nothing.  Must be the same on every rank.
        self.pool_last_block_long = env_flag("UNIIR_POOL_LAST_BLOCK_LONG")
        # The backward of ln_2 / ln_1 inside the launch of the c_fc / in_proj weight gradient (uniir_clip_tower.ln_bwd_side,
        # csrc/gemm.hip gemm_wgrad_side_kernel): the LayerNorm rows stream through a few compute units while the others feed the matrix
        # pipes.  Same activation gradients bit for bit; the two weight gradients and the LayerNorm parameter gradients are other
        # fixed-order fp32 sums.  UNIIR_LN_BWD_SIDE=0 runs the separate launches (A/B, tests).  Must be the same on every rank.
        self.ln_bwd_side = os.environ.get("UNIIR_LN_BWD_SIDE", "1") != "0"
        # Activation recomputation in the C towers (uniir_clip_tower.recompute, csrc/tower.hip): the training forward keeps only the
        # fp32 residual stream that enters each block (4 of the 28 - 36 stashed bytes per row x width element per layer) and the
        # backward rebuilds each block's intermediates from it, with the forward's own launches, right before that block's backward.
        # Bitwise the results of the stored run with stash_act = True (act(f) exists once in the shared layer buffers, so stash_act
        # has nothing to decide here); costs one more pass over the blocks' sublayers minus their c_proj GEMM per step.  For batches
        # whose stash does not fit.  UNIIR_RECOMPUTE_BLOCKS=1 switches it on at construction; must be the same on every rank.
        self.recompute_blocks = env_flag("UNIIR_RECOMPUTE_BLOCKS")
        self._recompute_logged = set()    # towers whose "recomputation is on" line is in stash_log already
        self._full_last_logged = set()    # towers whose "full last block" / "pooled last block above 512 tokens" line is in stash_log already
        self.stash_margin_bytes = 16 << 30
        self.stash_review_headroom_bytes = 6 << 30
        self._stash_choice = {}           # tower -> bool: the automatic decision, made once (at the first training batch)
        self.stash_log = []               # human-readable record of every decision (bench.py prints it)
        self.last_stash_act = {}          # tower -> what the last training forward chose
        self.last_text_rows = None      # (live rows, dense rows) of the last packed text-tower call (bench: executed FLOPs)
        # The two towers of a batch are independent until the fusion: with overlap_towers the TEXT leg of a model forward (side_leg()
        # in clip_sf.encode_multimodal_input) is enqueued on a second HIP stream and joined before the fusion; autograd runs the
        # leg's backward on that stream again (nodes run on the stream of their forward) and the tower backward joins it to the
        # stream the leg forked from.  The text tower's small GEMMs (1.6 rounds of 256-tiles at 35 k rows) then run on the compute
        # units the image tower's kernels leave idle in their last round of tiles and between launches.  No kernel changes and the
        # towers' buffers are disjoint (split-K slabs and workspaces are per tower): losses and embeddings are bitwise those of the
        # one-stream order, gradients equal up to the order of the fp32 atomic column sums, which neither order fixes.
        # True / False = forced (UNIIR_OVERLAP_TOWERS=1 / 0); None = automatic: ON in a single-rank job, OFF when a process group
        # with more than one rank exists.  With W > 1 the overlapped gradient reducer (comm.GradReducer) hands ranges to the
        # collective library from whichever stream announces them, and RCCL's async all-reduce orders against the CURRENT stream only:
        # that ordering has run over gloo (host copies, synchronous) but never over RCCL -- no two-GPU box in this environment -- so
        # a multi-rank job keeps the one-stream order until it has (bench.py --overlap-towers forces it for an A/B).
        env = os.environ.get("UNIIR_OVERLAP_TOWERS")
        self.overlap_towers = None if env is None else env != "0"
        self._side_streams = _SIDE_STREAMS          # one second stream per DEVICE, shared by every model of the process
        self._leg_main = None           # inside side_leg(): the stream the leg forked from

    # ---- flat parameter / gradient / bf16-shadow storage -----------------------------------------------------
    def _flat_order(self):
        """(name, parameter) in flat-buffer order: the no-decay tensors, then the decay tensors, each in named_parameters() order --
        NativeAdamW's two groups are two ranges, and a residual block's four weight matrices are adjacent (layer_grad_range)"""
        params = list(self.named_parameters())
        return [(n, p) for n, p in params if _is_no_decay(n, p)] + [(n, p) for n, p in params if not _is_no_decay(n, p)]

    def _ensure_flat(self):
        dev = self.logit_scale.device
        if dev.type != "cuda":
            raise RuntimeError("uniir_amd CLIP runs on an MI355X only (no CPU path); move the model to cuda")
        if self._flat is not None and self._flat.holds(self.named_parameters()):
            return self._flat
        self._flat = st = FlatStore.adopt(self._flat_order(), dev)
        st.add_padded(CONV, self.cfg["vision_width"], 3 * self.cfg["vision_patch_size"] ** 2, self.kpad)
        # tower_desc() cache: raw pointers into this store.  They stay valid for the store's life: its buffers, the fp16 shadow and the
        # padded copies included, are allocated once and refilled in place (FlatStore.half_shadow)
        self._descs = {}
        st.refresh_shadow()
        return st

    def refresh_shadow(self):
        """the 16-bit copies of the master weights follow a torch-side write (FlatStore.refresh_shadow; _sync_shadow() finds out by
        itself, and the fused AdamW tells the store)"""
        self._flat.refresh_shadow()

    def _sync_shadow(self):
        """the store, its bf16 copies up to date; the fp16 ones on top: _sync_shadow().half_shadow()"""
        st = self._ensure_flat()
        st.sync()
        return st

    def optimizer_groups(self):
        """(no-decay params, decay params): NativeAdamW's param groups 0 and 1 (clip_scorefusion/train.py:195-199)"""
        named = list(self.named_parameters())
        return [p for n, p in named if _is_no_decay(n, p)], [p for n, p in named if not _is_no_decay(n, p)]

    def adamw_group(self, name):
        """NativeAdamW's param group of tensor `name`"""
        return 0 if _is_no_decay(name, self.get_parameter(name)) else 1

    def w16(self, name):
        return self._flat.w16(name)

    def pool_last_value(self):
        """uniir_clip_tower.pool_last_block as the towers get it: 0 = every row through the last block, 1 = the pooled last block up to
        512 tokens (the full block above), 2 = the pooled last block at every token count (pool_last_block_long)"""
        if not self.pool_last_block:
            return 0
        return 2 if self.pool_last_block_long else 1

    def tower_desc(self, which, half=False):
        """the POD description uniir_clip_tower_{fwd,bwd} take (include/uniir_hip.h [TOWER]): raw device pointers into the flat
        fp32 / bf16-shadow / gradient buffers; cached until the flat storage is rebuilt.  half: the fp16 forward's description
        (dtype16 = 1, 16-bit weights from the store's fp16 shadow, which the caller has brought up to date)"""
        from ._lib import ClipBlock, ClipTower
        key = (which, bool(half))
        if key in self._descs:
            return self._descs[key][0]
        cfg, st = self.cfg, self._flat
        w16 = st.half_shadow() if half else st.w16_buf

        def p(name):
            return st.ptr(st.p32, name)

        def h(name):
            return st.ptr(w16, name)

        def g(name):
            return st.ptr(st.g32, name)

        image = which == "image"
        prefix = "visual.transformer" if image else "transformer"
        L = cfg["vision_layers"] if image else cfg["transformer_layers"]
        W = cfg["vision_width"] if image else cfg["transformer_width"]
        blocks = (ClipBlock * L)()
        for i in range(L):
            b, r = blocks[i], f"{prefix}.resblocks.{i}"
            b.ln1_w, b.ln1_b, b.ln2_w, b.ln2_b = p(f"{r}.ln_1.weight"), p(f"{r}.ln_1.bias"), p(f"{r}.ln_2.weight"), p(f"{r}.ln_2.bias")
            b.wqkv16, b.wo16 = h(f"{r}.attn.in_proj_weight"), h(f"{r}.attn.out_proj.weight")
            b.wfc16, b.wproj16 = h(f"{r}.mlp.c_fc.weight"), h(f"{r}.mlp.c_proj.weight")
            b.bqkv, b.bo = p(f"{r}.attn.in_proj_bias"), p(f"{r}.attn.out_proj.bias")
            b.bfc, b.bproj = p(f"{r}.mlp.c_fc.bias"), p(f"{r}.mlp.c_proj.bias")
            b.g_ln1_w, b.g_ln1_b, b.g_ln2_w, b.g_ln2_b = g(f"{r}.ln_1.weight"), g(f"{r}.ln_1.bias"), g(f"{r}.ln_2.weight"), g(f"{r}.ln_2.bias")
            b.g_wqkv, b.g_bqkv = g(f"{r}.attn.in_proj_weight"), g(f"{r}.attn.in_proj_bias")
            b.g_wo, b.g_bo = g(f"{r}.attn.out_proj.weight"), g(f"{r}.attn.out_proj.bias")
            b.g_wfc, b.g_bfc = g(f"{r}.mlp.c_fc.weight"), g(f"{r}.mlp.c_fc.bias")
            b.g_wproj, b.g_bproj = g(f"{r}.mlp.c_proj.weight"), g(f"{r}.mlp.c_proj.bias")
        t = ClipTower()
        t.dtype16 = int(bool(half))
        t.is_text, t.layers, t.width, t.embed_dim = int(not image), L, W, cfg["embed_dim"]
        t.blocks = C.cast(blocks, C.POINTER(ClipBlock))
        # split-K slabs: one scratch buffer PER TOWER (the two towers may run on two streams at the same time)
        # (ln_bwd_side: the c_fc gradient beside ln_2's backward is 13 slabs of 4W x W floats -- 218 MB at W = 1024)
        skw = ops._splitk_workspace(st.dev, max(128 << 20, 4 * 13 * 4 * W * W if self.ln_bwd_side else 0), tag=which)
        t.splitk_ws, t.splitk_ws_bytes = skw.data_ptr(), skw.numel()
        if image:
            P = cfg["vision_patch_size"]
            t.heads, t.tokens = W // 64, (cfg["image_resolution"] // P) ** 2 + 1
            t.resolution, t.patch, t.kpad = cfg["image_resolution"], P, self.kpad
            t.conv16 = (st.padded16h(CONV) if half else st.padded16(CONV)).data_ptr()
            t.class_emb, t.pos_emb = p("visual.class_embedding"), p("visual.positional_embedding")
            t.ln_pre_w, t.ln_pre_b = p("visual.ln_pre.weight"), p("visual.ln_pre.bias")
            t.ln_post_w, t.ln_post_b, t.proj16 = p("visual.ln_post.weight"), p("visual.ln_post.bias"), h("visual.proj")
            t.g_conv, t.g_class, t.g_pos = g("visual.conv1.weight"), g("visual.class_embedding"), g("visual.positional_embedding")
            t.g_ln_pre_w, t.g_ln_pre_b = g("visual.ln_pre.weight"), g("visual.ln_pre.bias")
            t.g_ln_post_w, t.g_ln_post_b, t.g_proj = g("visual.ln_post.weight"), g("visual.ln_post.bias"), g("visual.proj")
        else:
            t.heads, t.tokens, t.vocab = cfg["transformer_heads"], cfg["context_length"], cfg["vocab_size"]
            t.pos_emb, t.token_emb = p("positional_embedding"), p("token_embedding.weight")
            t.ln_post_w, t.ln_post_b, t.proj16 = p("ln_final.weight"), p("ln_final.bias"), h("text_projection")
            t.g_pos, t.g_token = g("positional_embedding"), g("token_embedding.weight")
            t.g_ln_post_w, t.g_ln_post_b, t.g_proj = g("ln_final.weight"), g("ln_final.bias"), g("text_projection")
        self._descs[key] = (t, blocks, skw)          # keep the host array and the scratch alive with the description
        return t

    def layer_grad_range(self, prefix, i):
        """[lo, hi) of the flat buffers that holds the four weight matrices of residual block i (adjacent: the weight-decay
        section keeps named_parameters() order and the block's gains / biases live in the other section)"""
        return self._flat.span([f"{prefix}.resblocks.{i}.{n}" for n in ("attn.in_proj_weight", "attn.out_proj.weight",
                                                                        "mlp.c_fc.weight", "mlp.c_proj.weight")])

    def block_done(self, prefix):
        """DDP overlap: with a gradient reducer armed (trainer.NativeAdamW.arm_overlap), the callable a backward of the tower `prefix`
        calls once residual block i is finished -- it hands the block's weight gradients to the collective stream while the
        remaining blocks still run; None when no reducer is armed"""
        reducer = getattr(self, "_grad_reducer", None)
        return None if reducer is None else (lambda i: reducer.ready(*self.layer_grad_range(prefix, i)))

    def zero_grad(self, set_to_none=False):
        """Gradients live in one flat buffer; zeroing it is one memset (they are never set to None)."""
        if self._flat is not None:
            self._flat.zero_grad(self.named_parameters())
        else:
            super().zero_grad(set_to_none=set_to_none)

    def review_stash(self, all_reduce_min=None):
        """Call after the first COMPLETE training step (trainer.NativeTrainer does): the automatic act(f) stash was sized before the
        first backward, i.e. before RCCL's channel buffers, the reducer's in-flight buckets and the optimizer state existed.  If the
        step's measured peak (torch's peak + what lives outside torch's allocator on this device) leaves less than
        stash_review_headroom_bytes of the device, the stash is switched off for the following steps -- on EVERY rank when
        all_reduce_min (a callable reducing a python float with MIN over the ranks) is given, so that replicas keep computing bitwise
        the same gradients.  Returns the headroom in bytes (None when nothing was decided automatically)."""
        # Only RANK-UNIFORM conditions may return before the collectives: the automatic decision itself is per rank (each rank's own
        # free memory, an out-of-memory re-plan), so a rank that chose "off" for every tower must still take part in both reductions
        # -- skipping them would leave its peers' MIN all-reduces to pair with this rank's next gradient bucket.
        if self.stash_act is not None or self._flat is None:
            return None
        # recompute_blocks: nothing to review (no act(f) stash exists); like a rank whose choice is "off", it still takes part in both
        # reductions, so the ranks stay paired whatever their peers run
        mine = any(self._stash_choice.values()) and not self.recompute_blocks
        if all_reduce_min is None and not mine:
            return None
        headroom, peak, outside = self._measured_headroom() if mine else (float("inf"), 0.0, 0.0)
        agreed = 1.0 if (mine and all(self._stash_choice.values())) else 0.0
        if all_reduce_min is not None:          # one mode on every rank from here on
            headroom = float(all_reduce_min(headroom))
            agreed = float(all_reduce_min(agreed))
        if not mine:
            if self._stash_choice and not self.recompute_blocks:
                self.stash_log.append("act(f) stash was off on this rank already; took part in the ranks' review")
            return None
        if headroom < self.stash_review_headroom_bytes or agreed == 0.0:
            for k in self._stash_choice:
                self._stash_choice[k] = False
            self.stash_log.append(f"act(f) stash switched off after the first step: measured headroom {headroom / 2**30:.1f} GiB "
                                  f"(floor {self.stash_review_headroom_bytes / 2**30:.0f} GiB), ranks agreed on the stash: {bool(agreed)}")
        else:
            self.stash_log.append(f"act(f) stash kept after the first step: measured headroom {headroom / 2**30:.1f} GiB "
                                  f"(peak {peak / 2**30:.1f} GiB in torch, {outside / 2**30:.1f} GiB outside)")
        return headroom

    def _measured_headroom(self):
        """(bytes of the device the finished step left unused at its peak, torch's peak, bytes held outside torch's allocator)"""
        dev = self._flat.dev
        free, total = torch.cuda.mem_get_info(dev)
        outside = total - free - torch.cuda.memory_reserved(dev)          # other processes / RCCL / HIP runtime on this device
        peak = torch.cuda.max_memory_allocated(dev)
        return float(total - outside - peak), float(peak), float(outside)

    # ---- two-stream towers -------------------------------------------------------------------------------------------
    def overlap_on(self):
        """overlap_towers resolved: forced value, or (automatic) on exactly when this is a single-rank job"""
        if self.overlap_towers is not None:
            return bool(self.overlap_towers)
        import torch.distributed as dist
        return not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1)

    @contextlib.contextmanager
    def side_leg(self, dev):
        """with model.side_leg(dev) as leg: everything enqueued inside (one tower call and the torch ops around it) goes to this
        model's second stream of `dev`, ordered after all work enqueued so far on the current stream; leg is None when the overlap is
        off (CPU tensors, overlap_towers False) and the body then runs on the current stream as before.
        The caller hands the tensors the leg produced to join_leg() before the current stream reads them."""
        dev = torch.device(dev)
        if not self.overlap_on() or dev.type != "cuda" or self.precision == "fp32" or self._leg_main is not None:
            yield None
            return
        # every lazily built shared buffer (flat storage, 16-bit shadows of the weights) is brought up to date on the forking stream,
        # BEFORE the fork: both towers read them
        st = self._sync_shadow()
        if self.precision == "fp16":
            st.half_shadow()
        main = torch.cuda.current_stream(dev)
        side = self._side_streams.get(dev.index)
        if side is None:
            side = self._side_streams[dev.index] = torch.cuda.Stream(dev)
        side.wait_stream(main)
        self._leg_main = main
        try:
            with torch.cuda.stream(side):
                yield side
        finally:
            self._leg_main = None

    @staticmethod
    def join_leg(leg, *tensors):
        """the current stream waits for everything side_leg() enqueued; `tensors` (allocated inside the leg) are about to be read on
        the current stream"""
        if leg is None:
            return
        main = torch.cuda.current_stream(leg.device)
        main.wait_stream(leg)
        for t in tensors:
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(main)

    # ---- public encoder API (upstream names) ---------------------------------------------------------------------
    @property
    def dtype(self):
        return torch.float32

    def encode_image(self, image):
        self._sync_shadow()
        return _TowerFn.apply(self, "image", image.contiguous(), self._anchor_for(image.device))

    def encode_text(self, text):
        self._sync_shadow()
        tok = text.to(torch.int32).contiguous()
        if self.pack_text and tok is not text:       # the caller's tensor object carries the remembered row offsets
            ver = _tensor_version(tok)
            if ver is not None:
                tok._uniir_row_off = (ver, tuple(tok.shape), text_row_offsets(text))
        return _TowerFn.apply(self, "text", tok, self._anchor_for(text.device))

    def _anchor_for(self, dev):
        # a leaf that requires grad, so autograd calls the tower backward (parameter grads are written straight
        # into the flat gradient buffer, they do not travel through autograd)
        return torch.zeros(1, device=dev, requires_grad=torch.is_grad_enabled())


# ------------------------------------------------------------------------------------------------------------
# fp32 forward (precision = "fp32"): the same block sequence on the fp32 launch layer (fp32_forward.py).  openai/CLIP model.py
# semantics as restated in SURVEY.md 3.2.
# ------------------------------------------------------------------------------------------------------------
def image_blocks_f32(model, image):
    """the vision tower up to its last residual block, every token: image [M,3,res,res] -> x fp32 [M*T, W], T"""
    cfg, p32 = model.cfg, model._flat.p
    W, M = cfg["vision_width"], image.shape[0]
    x0, T = patch_tokens_f32(image, cfg["vision_patch_size"], p32("visual.conv1.weight"), None, p32("visual.class_embedding"),
                             p32("visual.positional_embedding"))
    x = layernorm_f32(x0, p32("visual.ln_pre.weight"), p32("visual.ln_pre.bias"))
    return tower_fwd_f32(p32, lambda i: clip_block_names("visual.transformer", i), cfg["vision_layers"], x, M, T, W, W // 64, False), T


def text_blocks_f32(model, text):
    """the text tower up to its last residual block, every token: text int32 [M,ctx] -> x fp32 [M*T, W], the EOT positions, T"""
    cfg, p32 = model.cfg, model._flat.p
    dev, M = text.device, text.shape[0]
    W, L, T = cfg["transformer_width"], cfg["transformer_layers"], cfg["context_length"]
    x = torch.empty(M * T, W, device=dev, dtype=torch.float32)
    eot = torch.empty(M, device=dev, dtype=torch.int32)
    ops.call("uniir_text_embed", text, p32("token_embedding.weight"), p32("positional_embedding"), x, eot, M, T, W,
             cfg["vocab_size"])
    return tower_fwd_f32(p32, lambda i: clip_block_names("transformer", i), L, x, M, T, W, cfg["transformer_heads"], True), eot, T


def _encode_fp32(model, which, inp, p32):
    M = inp.shape[0]
    if which == "image":
        (x, T), eot = image_blocks_f32(model, inp), None
        lnw, lnb, proj = "visual.ln_post.weight", "visual.ln_post.bias", "visual.proj"
    else:
        x, eot, T = text_blocks_f32(model, inp)
        lnw, lnb, proj = "ln_final.weight", "ln_final.bias", "text_projection"
    rows = torch.empty(M, x.shape[1], device=inp.device, dtype=torch.float32)
    ops.call("uniir_gather_rows", x, eot, rows, M, T, x.shape[1])
    return linear_f32(layernorm_f32(rows, p32(lnw), p32(lnb)), p32(proj), w_kn=True)          # pooled @ proj, proj [W, E]


def _join_backward(st, demb):
    """a tower backward that ran on the side stream of CLIP.side_leg(): its parameter gradients went straight into the flat gradient
    buffer (no AccumulateGrad node the autograd engine could synchronise on), so the stream the leg forked from -- where the optimizer,
    the gradient reducer's finish() and the next step's zero_grad run -- waits for it here.  Autograd runs the later-built image tower
    backward first, so at this point the whole image backward is already enqueued on that stream and nothing of it is delayed."""
    main = st.get("join_to")
    if main is None:
        return
    cur = torch.cuda.current_stream(demb.device)
    if cur != main:
        demb.record_stream(cur)
        main.wait_stream(cur)


class _TowerFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, which, inp, anchor):
        cfg = model.cfg
        need_grad = bool(ctx.needs_input_grad[3])
        dev = inp.device
        E = cfg["embed_dim"]
        M = inp.shape[0]
        ctx.model, ctx.which, ctx.M = model, which, M
        if M == 0:
            return torch.zeros(0, E, device=dev)
        if model.precision == "fp32":
            if need_grad:
                raise RuntimeError("precision='fp32' is a forward-only path (embedding extraction / parity); run it under "
                                   "torch.no_grad() or switch back to precision='bf16' for training")
            return _encode_fp32(model, which, inp, model._flat.p)
        half = model.precision == "fp16"
        if half:
            if need_grad:
                raise RuntimeError("precision='fp16' is the embedder's forward-only path; run it under torch.no_grad() or switch "
                                   "back to precision='bf16' for training")
            model._sync_shadow().half_shadow()
        elif model.precision != "bf16":
            raise RuntimeError(f"unknown precision {model.precision!r}")
        # the whole tower in one C call (csrc/tower.hip); the workspace is the activation stash of the backward
        lib = _lib.load()
        desc = model.tower_desc(which, half=half)
        desc.pool_last_block = model.pool_last_value()
        if desc.pool_last_block and desc.tokens > ops.ATT_RESIDENT_MAX and (which, desc.pool_last_block) not in model._full_last_logged:
            model._full_last_logged.add((which, desc.pool_last_block))
            if desc.pool_last_block == 2:
                model.stash_log.append(f"{which} tower, {desc.tokens} tokens: pooled last block on the one-query streaming path "
                                       f"(pool_last_block_long): same embeddings, 1/{desc.layers} less block work")
            else:
                # (csrc/tower.hip plan(): the resident one-query attention of the pooled block holds all keys in LDS, 512 at the most)
                model.stash_log.append(f"{which} tower, {desc.tokens} tokens: full last block (pool_last_block needs <= {ops.ATT_RESIDENT_MAX} tokens); "
                                       f"same embeddings, 1/{desc.layers} more block work")
        # recompute_blocks: only the block inputs are kept (uniir_clip_tower.recompute); a forward-only call has no stash to shrink
        recompute = need_grad and bool(model.recompute_blocks)
        desc.recompute = int(recompute)
        emb = torch.empty(M, E, device=dev, dtype=torch.float32)

        def ws_bytes(stash):
            desc.stash_act = int(stash)
            if which == "text" and model.pack_text:
                return lib.uniir_clip_tower_workspace_bytes_packed(C.byref(desc), M, text_row_offsets(inp)[1], int(need_grad))
            return lib.uniir_clip_tower_workspace_bytes(C.byref(desc), M, int(need_grad))

        stash = False
        auto = False
        if recompute:       # act(f) lives once in the shared layer buffers: the stash_act = 1 arithmetic, nothing to decide or re-plan
            stash = True
        elif need_grad and model.stash_act is not False:
            stash = True
            if model.stash_act is None:        # automatic: decided once per (tower, batch), see CLIP.__init__
                auto = True
                key = which
                if key not in model._stash_choice:
                    free, _ = torch.cuda.mem_get_info(dev)
                    avail = free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
                    need_stash = ws_bytes(True)
                    model._stash_choice[key] = need_stash + model.stash_margin_bytes <= avail
                    model.stash_log.append(f"{which} tower, {M} items: act(f) stash {'ON' if model._stash_choice[key] else 'off'} "
                                           f"(workspace {need_stash / 2**30:.1f} GiB, {avail / 2**30:.1f} GiB available, margin "
                                           f"{model.stash_margin_bytes / 2**30:.0f} GiB)")
                stash = model._stash_choice[key]
        desc.stash_act = int(stash)
        model.last_stash_act[which] = bool(stash)

        def alloc_ws(nbytes_of):
            """the tower workspace; when the automatic act(f) stash does not fit after all, re-plan this tower without it"""
            nonlocal stash

            def attempt():
                n = nbytes_of()
                return n, (torch.empty(n, device=dev, dtype=torch.uint8) if n >= 0 else None)

            try:
                try:
                    return attempt()
                except torch.OutOfMemoryError:
                    if not (auto and stash):
                        raise
                    torch.cuda.empty_cache()
                    stash = False
                    model._stash_choice[which] = False
                    model.last_stash_act[which] = False
                    desc.stash_act = 0
                    model.stash_log.append(f"{which} tower, {M} items: act(f) stash dropped after an out-of-memory error on its allocation")
                    return attempt()
            except torch.OutOfMemoryError as e:
                if not need_grad or recompute:
                    raise
                n_stored = nbytes_of()          # the stored-mode stash does not fit for good: name the mode that needs less
                desc.recompute = 1
                n_rc = nbytes_of()
                desc.recompute = 0
                raise torch.OutOfMemoryError(
                    f"{which} tower, {M} items: the activation stash of the training forward ({n_stored / 2**30:.1f} GiB) does not fit. "
                    f"Activation recomputation (CLIP.recompute_blocks = True, or UNIIR_RECOMPUTE_BLOCKS=1) keeps only the block inputs "
                    f"and needs {n_rc} bytes ({n_rc / 2**30:.1f} GiB) for this tower, at the cost of one more pass over the blocks "
                    f"per step. ({e})") from e

        def log_recompute(n):
            if recompute and which not in model._recompute_logged:
                model._recompute_logged.add(which)
                model.stash_log.append(f"{which} tower, {M} items: block recomputation ON (recompute_blocks): workspace {n} bytes "
                                       f"({n / 2**30:.1f} GiB), block inputs only; act(f) stash not applicable")

        if which == "text" and model.pack_text:
            # exact packing: only the tokens up to each caption's EOT are rows of the text tower (text_row_offsets)
            row_off, live = text_row_offsets(inp)
            need, ws = alloc_ws(lambda: lib.uniir_clip_tower_workspace_bytes_packed(C.byref(desc), M, live, int(need_grad)))
            if need < 0:
                raise RuntimeError("uniir_clip_tower: unsupported tower geometry")
            log_recompute(need)
            _lib.check(lib.uniir_clip_tower_fwd_packed(C.byref(desc), inp.data_ptr(), M, row_off.data_ptr(), live, emb.data_ptr(),
                                                       ws.data_ptr(), need, int(need_grad), ops._stream()), "clip_tower_fwd_packed")
            model.last_text_rows = (live, M * cfg["context_length"])
            if need_grad:
                ctx.stash = dict(ws=ws, inp=inp, row_off=row_off, live=live, stash_act=int(stash), join_to=model._leg_main,
                                 pool_last=int(desc.pool_last_block), recompute=int(recompute))
            return emb
        need, ws = alloc_ws(lambda: lib.uniir_clip_tower_workspace_bytes(C.byref(desc), M, int(need_grad)))
        if need < 0:
            raise RuntimeError("uniir_clip_tower: unsupported tower geometry")
        log_recompute(need)
        inp = inp.float().contiguous() if which == "image" else inp
        _lib.check(lib.uniir_clip_tower_fwd(C.byref(desc), inp.data_ptr(), M, emb.data_ptr(), ws.data_ptr(), need,
                                            int(need_grad), ops._stream()), "clip_tower_fwd")
        if need_grad:
            ctx.stash = dict(ws=ws, inp=inp, stash_act=int(stash), join_to=model._leg_main,
                             pool_last=int(desc.pool_last_block), recompute=int(recompute))
        return emb

    @staticmethod
    def backward(ctx, demb):
        model, which, M = ctx.model, ctx.which, ctx.M
        if M == 0:
            return None, None, None, None
        st = ctx.stash
        ctx.stash = None
        lib = _lib.load()
        desc = model.tower_desc(which)
        desc.stash_act = st["stash_act"]        # part of the workspace layout: the value the forward ran with
        desc.pool_last_block = st["pool_last"]
        desc.recompute = st["recompute"]
        desc.ln_bwd_side = int(bool(model.ln_bwd_side))      # (not part of the workspace layout)
        ws, inp, stream = st["ws"], st["inp"], ops._stream()
        demb = demb.contiguous().float()
        need = ws.numel()
        L = desc.layers
        block_done = model.block_done("visual.transformer" if which == "image" else "transformer")
        if "row_off" in st:         # the text tower on packed rows
            ro, live = st["row_off"].data_ptr(), st["live"]
            _lib.check(lib.uniir_clip_tower_bwd_head_packed(C.byref(desc), demb.data_ptr(), M, ro, live, ws.data_ptr(), need, stream),
                       "tower_bwd_head_packed")
            for lo, hi in ([(0, L)] if block_done is None else [(i, i + 1) for i in reversed(range(L))]):
                _lib.check(lib.uniir_clip_tower_bwd_blocks_packed(C.byref(desc), M, ro, live, lo, hi, ws.data_ptr(), need, stream),
                           "tower_bwd_blocks_packed")
                if block_done is not None:
                    block_done(lo)
            _lib.check(lib.uniir_clip_tower_bwd_stem_packed(C.byref(desc), inp.data_ptr(), M, ro, live, ws.data_ptr(), need, stream),
                       "tower_bwd_stem_packed")
            _join_backward(st, demb)
            return None, None, None, None
        _lib.check(lib.uniir_clip_tower_bwd_head(C.byref(desc), demb.data_ptr(), M, ws.data_ptr(), need, stream), "tower_bwd_head")
        if block_done is None:
            _lib.check(lib.uniir_clip_tower_bwd_blocks(C.byref(desc), M, 0, L, ws.data_ptr(), need, stream), "tower_bwd_blocks")
        else:       # DDP overlap: hand every finished block's weight gradients to the collective stream
            for i in reversed(range(L)):
                _lib.check(lib.uniir_clip_tower_bwd_blocks(C.byref(desc), M, i, i + 1, ws.data_ptr(), need, stream),
                           "tower_bwd_blocks")
                block_done(i)
        _lib.check(lib.uniir_clip_tower_bwd_stem(C.byref(desc), inp.data_ptr(), M, ws.data_ptr(), need, stream), "tower_bwd_stem")
        _join_backward(st, demb)
        return None, None, None, None
