"""The precision of an embedding forward, stated once for every model that carries one (clip_model.CLIP, BLIPFeatureFusion /
BLIPScoreFusion, CLIPFeatureFusion).  Three plain attributes, which a constructor sets and anyone may change between calls:

  precision   "bf16": the MFMA kernels of training, forward and backward.  "fp16": the same launch sequence on fp16 activations and fp16
              copies of the weights, FORWARD ONLY -- the reference embedder's autocast(fp16) (mbeir_embedder.py:52-56), the bf16 rate,
              3 more mantissa bits: embeddings 1e-3 from the fp32 oracle instead of 6e-3.  "fp32": the reference's model.float() forward
              -- what an embed YAML with use_fp16: False means -- in exact-fp32 MFMA GEMMs, fp32 attention and norms on the fp32 masters
              (fp32_forward.py), forward only; reference precision, not throughput (profiles/embed_fp32.txt).
  embed_fp16  whether the embedder's use_fp16: True switches a "bf16" module to "fp16" for an extraction (src/common/mbeir_embedder.py
              _tower_precision).  BLIP and CLIP_FF: off unless UNIIR_BLIP_EMBED_FP16=1 / UNIIR_CLIPFF_EMBED_FP16=1 at construction.  The
              CLIP module has no such attribute: its towers always took fp16 under use_fp16.
  embed_fp32  whether the embedder's use_fp16: False switches a "bf16" module to "fp32" in the same way: off unless UNIIR_EMBED_FP32=1
              at construction.  On BLIP and CLIP_FF it is also what makes "fp32" a precision the module knows: without it "fp32" raises
              `unknown precision`, so a model that has not opted in behaves in every respect as it did before the fp32 forward existed.

pool_fp32() is the storage switch that goes with embed_fp32: UNIIR_POOL_FP32=1, read when used.  With it an extraction under
use_fp16: False keeps its fp32 rows (the .npy, the .index container, the resident shards) and the search runs on them
(uniir_topk_ip_f32: the oracle's arithmetic over fp32 rows); without it, or under use_fp16: True, every row is rounded to fp16 as
before and every file keeps its bytes.

embed_mode() is the rule of an encode call of BLIP and CLIP_FF.  clip_model._TowerFn keeps its own three lines: the C towers ask
whether THIS call records a backward (needs_input_grad), not for grad mode, know no train-mode guard and no opt-in, so routing them
through embed_mode() would take a flag per guard."""
import os

import torch

PRECISIONS = ("bf16", "fp16", "fp32")


def env_flag(name):
    """an opt-in switch of the environment: set, and neither empty nor "0" """
    return os.environ.get(name, "0") not in ("", "0")


def pool_fp32():
    """keep (and search) fp32 embedding rows where use_fp16 is False: UNIIR_POOL_FP32=1, read at every use"""
    return env_flag("UNIIR_POOL_FP32")


def check_mode(mode, known, training, hint=""):
    """`mode` is one of `known`, and anything but "bf16" is an eval-mode path"""
    if mode not in known:
        raise RuntimeError(f"unknown precision {mode!r}" + (hint if mode == "fp32" else ""))
    if mode != "bf16" and training:
        raise RuntimeError(f"precision='{mode}' is a forward-only embedding path; call model.eval() first or use precision='bf16'")


def embed_mode(module, *, use_momentum=False, fp16_refuses_grad=False):
    """the precision of this encode call of `module`: "bf16", or the forward-only embedding path "fp16" / "fp32"; what that path cannot
    serve raises, before any launch.  use_momentum: the call asks for BLIP's momentum encoder.  fp16_refuses_grad: CLIP_FF's fp16 goes
    through its autograd function and so needs torch.no_grad(); BLIP's wraps itself in it.  "fp32" always needs it."""
    mode = module.precision
    check_mode(mode, PRECISIONS if module.embed_fp32 else PRECISIONS[:2], module.training,
               " for a model that has not opted in to the fp32 embedding forward: set embed_fp32 = True (UNIIR_EMBED_FP32=1 at "
               "construction) first")
    if mode == "bf16":
        return mode
    if use_momentum:
        raise RuntimeError(f"precision='{mode}' is the online encoder's embedding path: the fp16 shadow and the fp32 forward exist for "
                           "the online store only (use_momentum=True needs precision='bf16')")
    if torch.is_grad_enabled() and (mode == "fp32" or fp16_refuses_grad):
        raise RuntimeError(f"precision='{mode}' is a forward-only path (embedding extraction / parity); run it under torch.no_grad() or "
                           "switch back to precision='bf16' for training")
    return mode
