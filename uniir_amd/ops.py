"""Tensor-level wrappers over the C ABI (include/uniir_hip.h).  PyTorch is only the device-memory / stream
plumbing here: every function passes raw device pointers + the current HIP stream to libuniir_hip.so.
There is no torch fallback: a CPU tensor raises."""
import ctypes as C
import os
import warnings

import torch

from . import _lib
from ._lib import GemmDesc, check

EPI_BF16, EPI_BIAS_ACT, EPI_RESID_F32, EPI_DACT, EPI_F32, EPI_ATOMIC_F32, EPI_ACT_ONLY = range(7)
ACT_QUICKGELU, ACT_GELU_ERF, ACT_RELU = range(3)
DT_BF16, DT_F16 = 0, 1
GEMM_TIMING_STRIDE = 29   # bench.py: every 29th uniir_gemm call is bracketed by HIP events inside the library (uniir_gemm_timing);
# 441 GEMM launches per step and 441 % 29 = 6, so the sampled positions walk through every shape within a few steps


def gemm_timing_start(stride=GEMM_TIMING_STRIDE, stream=None):
    """stream: a torch.cuda.Stream -- sample the launches on that stream only (the other tower's stream shares the device: an event
    pair there would measure shared time, see uniir_gemm_timing_on)"""
    if stream is None:
        check(_lib.load().uniir_gemm_timing(int(stride)), "gemm_timing")
    else:
        check(_lib.load().uniir_gemm_timing_on(int(stride), C.c_void_p(stream.cuda_stream)), "gemm_timing_on")


def gemm_timing_stop(with_shared=False):
    """-> (sum of 2 M N K, seconds, launches) over the sampled GEMM launches [, samples left out because another stream's GEMMs
    shared the device with them: gemm_timing_start(stream=...), and whether the rule fell back to all samples because fewer than 8
    would have been left]; synchronise the device first"""
    f, ms, n, sh, fb = C.c_double(), C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
    check(_lib.load().uniir_gemm_timing_read_ex(C.byref(f), C.byref(ms), C.byref(n), C.byref(sh), C.byref(fb)), "gemm_timing_read")
    check(_lib.load().uniir_gemm_timing(0), "gemm_timing")
    if with_shared:
        return f.value, ms.value * 1e-3, n.value, sh.value, bool(fb.value)
    return f.value, ms.value * 1e-3, n.value


def gemm_timing_filter(windows, samples, merge_ms=-1.0):
    """the sampling rule alone (host arithmetic, no device): windows [(begin, end) ms], samples [(begin, duration) ms] ->
    (keep flags, fell back to all samples?)"""
    nw, n = len(windows), len(samples)
    w = (C.c_float * max(1, 2 * nw))(*[x for p in windows for x in p])
    s = (C.c_float * max(1, 2 * n))(*[x for p in samples for x in p])
    keep, fb = (C.c_uint8 * max(1, n))(), C.c_int32()
    kept = _lib.load().uniir_gemm_timing_filter(w, nw, s, n, float(merge_ms), keep, C.byref(fb))
    if kept < 0:
        check(kept, "gemm_timing_filter")
    return [bool(keep[i]) for i in range(n)], bool(fb.value)



# Reproducible reductions (include/uniir_hip.h uniir_reduce_scratch): every stream this module launches on gets a scratch buffer, so
# that bias / LayerNorm / embedding / relative-position-bias gradients are added in a fixed order and two runs of one step give the
# same bits.  A reduction that asks for more than the buffer holds keeps its atomics for that launch and the library counts it
# (reduce_stats); the next launch on the stream finds the request in the library's max_request and grows the buffer, so at most the
# first step of a new geometry is added in arrival order, and the counter says when that was.
# UNIIR_DETERMINISTIC=0 registers no scratch: the kernels stay on their fp32 atomics (A/B of the extra reduce launches) and the
# counter simply counts.
RED_SCRATCH_BYTES = 64 << 20
_RED_SCRATCH = {}
_DETERMINISTIC = os.environ.get("UNIIR_DETERMINISTIC", "1") != "0"
_RED_REFUSED = {}          # (device, stream) -> the smallest size whose allocation failed: not tried again
# max_request is read before every launch, so the read is kept cheap: one word and one bound function for the module.  Python threads
# share the word, which is harmless: it holds a process-wide figure that only grows between resets, whoever read it last.
_RED_MAX = C.c_int64()
_RED_MAX_REF = C.byref(_RED_MAX)
_RED_STATS = None


def reduce_stats():
    """-> (fallbacks, max_request) of the process since the last reset: reduction launches that were added in arrival order (fp32
    atomics) because their stream had no scratch buffer or too small a one, and the largest scratch size any reduction asked for
    (bytes)"""
    f, m = C.c_int64(), C.c_int64()
    check(_lib.load().uniir_reduce_stats(C.byref(f), C.byref(m), 0), "reduce_stats")
    return f.value, m.value


def reset_reduce_stats():
    check(_lib.load().uniir_reduce_stats(None, None, 1), "reduce_stats")


def _register_scratch(s, nbytes):
    with torch.cuda.device(s.device), torch.cuda.stream(s):      # allocated ON the stream: the caching allocator hands the old
        buf = torch.empty(nbytes, dtype=torch.uint8, device=s.device)      # buffer's memory to later work of this stream only
        check(_lib.load().uniir_reduce_scratch(C.c_void_p(buf.data_ptr()), nbytes, C.c_void_p(s.cuda_stream)), "reduce_scratch")
    return buf


def _stream():
    s = torch.cuda.current_stream()
    if _DETERMINISTIC:
        key = (s.device.index, s.cuda_stream)
        buf = _RED_SCRATCH.get(key)
        if buf is None:
            if len(_RED_SCRATCH) >= 24:          # streams come and go (tests): forget the oldest entry -- in the library's table
                old = next(iter(_RED_SCRATCH))   # first, so that it never points at freed memory
                with torch.cuda.device(old[0]):
                    _lib.load().uniir_reduce_scratch(None, 0, C.c_void_p(old[1]))
                del _RED_SCRATCH[old]
                _RED_REFUSED.pop(old, None)
            buf = _RED_SCRATCH[key] = _register_scratch(s, RED_SCRATCH_BYTES)
        global _RED_STATS
        if _RED_STATS is None:
            _RED_STATS = _lib.load().uniir_reduce_stats
        _RED_STATS(None, _RED_MAX_REF, 0)
        need = _RED_MAX
        if need.value > buf.numel():             # some reduction did not fit (and kept its atomics): the next power of two
            nbytes = 1 << (need.value - 1).bit_length()
            if nbytes < _RED_REFUSED.get(key, nbytes + 1):
                try:
                    new = _register_scratch(s, nbytes)
                except torch.cuda.OutOfMemoryError:
                    # the old buffer stays registered; reductions of that size keep their atomics and stay counted
                    _RED_REFUSED[key] = nbytes
                    warnings.warn(f"uniir_amd: a reduction asked for {need.value} bytes of scratch, but {nbytes} bytes could not be "
                                  f"allocated for stream {s.cuda_stream:#x}; it stays in arrival order (ops.reduce_stats())",
                                  RuntimeWarning, stacklevel=3)
                else:
                    warnings.warn(f"uniir_amd: a reduction asked for {need.value} bytes of scratch; the buffer of stream "
                                  f"{s.cuda_stream:#x} grows from {buf.numel()} to {nbytes} bytes (launches before this one were "
                                  "added in arrival order, see ops.reduce_stats())", RuntimeWarning, stacklevel=3)
                    _RED_SCRATCH[key] = new
    return C.c_void_p(s.cuda_stream)


def _p(t):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError("uniir_amd ops need device tensors (no CPU fallback on the product path)")
    return C.c_void_p(t.data_ptr())


_SPLITK_WS = {}


def _splitk_workspace(device, nbytes, tag=None):
    """one reusable scratch buffer per (device, tag) for the split-K slabs (stream-ordered reuse: users that may run on
    different streams at the same time -- the two CLIP towers -- pass different tags)"""
    key = (device, tag)
    ws = _SPLITK_WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 128 << 20), device=device, dtype=torch.uint8)
        _SPLITK_WS[key] = ws
    return ws


def gemm(A, B, C_out, M, N, K, lda, ldb, ldc, *, a_tmaj=False, b_tmaj=False, epilogue=EPI_BF16, bias=None,
         resid=None, aux=None, ldaux=0, C2=None, act=ACT_QUICKGELU, k_splits=1, alpha=1.0, dtype=DT_BF16,
         colsum=None, row_scale=None, a_rowsum=None):
    d = GemmDesc()
    d.A, d.B, d.C, d.C2 = A.data_ptr(), B.data_ptr(), C_out.data_ptr(), (C2.data_ptr() if C2 is not None else None)
    d.bias = bias.data_ptr() if bias is not None else None
    d.resid = resid.data_ptr() if resid is not None else None
    d.aux = aux.data_ptr() if aux is not None else None
    d.M, d.N, d.K = M, N, K
    d.lda, d.ldb, d.ldc, d.ldaux = lda, ldb, ldc, ldaux
    d.a_tmaj, d.b_tmaj = int(a_tmaj), int(b_tmaj)
    d.epilogue, d.act, d.dtype, d.k_splits, d.alpha = epilogue, act, dtype, k_splits, alpha
    d.colsum = colsum.data_ptr() if colsum is not None else None
    d.row_scale = row_scale.data_ptr() if row_scale is not None else None
    d.a_rowsum = a_rowsum.data_ptr() if a_rowsum is not None else None
    if k_splits > 1:
        ws = _splitk_workspace(A.device, 4 * k_splits * M * N)
        d.splitk_ws, d.splitk_ws_bytes = ws.data_ptr(), ws.numel()
    check(_lib.load().uniir_gemm(C.byref(d), _stream()), "gemm")
    return C_out


def _dtype16(first, *rest):
    """DT_BF16 / DT_F16 of a call from its 16-bit operands (None entries skipped): they all have the type of `first`.  fp16 is the
    forward-only path of the embedding towers; mixing it with bf16 is a ValueError, raised before anything is launched"""
    half = first.dtype == torch.float16
    for t in rest:
        if t is not None and (t.dtype == torch.float16) != half:
            raise ValueError(f"mixed 16-bit operands: {first.dtype} with {t.dtype} (an fp16 call takes fp16 tensors only)")
    return DT_F16 if half else DT_BF16


def linear_fwd(x, w, bias=None, *, out=None, epilogue=EPI_BF16, resid=None, C2=None, act=ACT_QUICKGELU, row_scale=None):
    """y[M,N] = x[M,K] @ w[N,K]^T (+bias ...).  x, w bf16 contiguous.  row_scale (fp32 [M], EPI_RESID_F32): the branch output is
    multiplied by it before the residual is added (DropPath).
    The 16-bit type follows x: an fp16 x needs an fp16 w (ValueError otherwise), the product runs as UNIIR_DT_F16 and the 16-bit
    outputs are fp16 (the forward-only fp16 path; the library refuses the epilogues that have no fp16 form)."""
    M, K = x.shape
    N = w.shape[0]
    dt16 = _dtype16(x, w, *(() if epilogue in (EPI_RESID_F32, EPI_F32) else (out,)), C2)
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float32 if epilogue in (EPI_RESID_F32, EPI_F32) else x.dtype)
    return gemm(x, w, out, M, N, K, K, K, N, epilogue=epilogue, bias=bias, resid=resid, C2=C2, act=act, row_scale=row_scale,
                dtype=dt16)


def linear_dgrad(dy, w, *, out=None, aux=None, act=ACT_QUICKGELU, act_out=None, colsum=None):
    """dx[M,K] = dy[M,N] @ w[N,K]  (optionally * act'(aux)).
    act_out (bf16 [M,K]): also receives act(aux), the recomputed activation (needs aux).
    colsum (fp32 [K]): += column sums of dx (the bias gradient of the layer that produced aux).  With aux the library produces
    act_out and colsum itself whichever kernel the problem runs (fused in the 256-tile epilogue, separate passes otherwise);
    without aux the product has the plain bf16 epilogue, which takes no colsum: the colsum kernel sums the bf16 result."""
    M, N = dy.shape
    K = w.shape[1]
    if out is None:
        out = torch.empty(M, K, device=dy.device, dtype=torch.bfloat16)
    if act_out is not None and aux is None:
        raise ValueError("act_out needs aux")
    gemm(dy, w, out, M, K, N, N, K, K, b_tmaj=True, epilogue=EPI_DACT if aux is not None else EPI_BF16,
         aux=aux, ldaux=K, act=act, C2=act_out, colsum=colsum if aux is not None else None)
    if colsum is not None and aux is None:
        call("uniir_colsum_bf16", out, K, colsum, M, K)
    return out


def wgrad_splits(rows, tiles):
    """split-K factor for dW (256x256 output tiles): uniir_gemm_wgrad_splits, the rule the C towers use too"""
    return _lib.load().uniir_gemm_wgrad_splits(int(rows), int(tiles))


def linear_wgrad(dy, x, dw, *, dbias=None):
    """dw[N,K] (fp32) += dy[M,N]^T @ x[M,K];  dbias[N] (fp32) += column sums of dy (from the same pass over dy when the
    256x256 transposed kernel runs)."""
    M, N = dy.shape
    K = x.shape[1]
    tiles = ((N + 255) // 256) * ((K + 255) // 256)
    return gemm(dy, x, dw, N, K, M, N, K, K, a_tmaj=True, b_tmaj=True, epilogue=EPI_ATOMIC_F32,
                k_splits=wgrad_splits(M, tiles), a_rowsum=dbias)


def layernorm_fwd(x, gamma, beta, eps=1e-5, *, out_bf16=None, out_f32=None, rows=None, width=None, x_stride=None,
                  dtype16=torch.bfloat16):
    """out_bf16: the 16-bit output; an fp16 tensor there (or dtype16 = torch.float16 when this function allocates it) takes
    uniir_layernorm_fwd_f16 -- the same fp32 result, rounded to fp16 (the forward-only fp16 path)"""
    width = width or x.shape[-1]
    rows = rows if rows is not None else x.numel() // width
    x_stride = x_stride or width
    if out_bf16 is None and out_f32 is None:
        out_bf16 = torch.empty(rows, width, device=x.device, dtype=dtype16)
    if out_bf16 is not None and out_bf16.dtype == torch.float16:
        check(_lib.load().uniir_layernorm_fwd_f16(_p(x), x_stride, _p(gamma), _p(beta), _p(out_bf16), _p(out_f32), rows,
                                                  width, eps, _stream()), "layernorm_fwd_f16")
        return out_bf16
    check(_lib.load().uniir_layernorm_fwd(_p(x), x_stride, _p(gamma), _p(beta), _p(out_bf16), _p(out_f32), rows,
                                          width, eps, _stream()), "layernorm_fwd")
    return out_bf16 if out_bf16 is not None else out_f32


def layernorm_bwd(x, gamma, dy, dgamma, dbeta, eps=1e-5, *, dres=None, dx=None, dx_bf16=None, rows=None,
                  width=None, x_stride=None, dx_stride=None, dx_colsum=None, branch_scale=None):
    """dx_colsum (fp32 [width]): += column sums of dx (bias gradient of the linear layer that produced x).
    branch_scale (fp32 [rows]): dx_bf16 and dx_colsum carry branch_scale[row] * dx (DropPath of the branch dx enters next)"""
    width = width or x.shape[-1]
    rows = rows if rows is not None else x.numel() // width
    x_stride = x_stride or width
    dx_stride = dx_stride or width
    if dx is None:
        dx = torch.empty(rows, width, device=x.device, dtype=torch.float32)
    if branch_scale is not None:
        check(_lib.load().uniir_layernorm_bwd_ex(_p(x), x_stride, _p(gamma), _p(dy), int(dy.dtype == torch.float32),
                                                 _p(dres), _p(dx), dx_stride, _p(dx_bf16), _p(dgamma), _p(dbeta),
                                                 _p(dx_colsum), _p(branch_scale), rows, width, eps, _stream()), "layernorm_bwd_ex")
        return dx
    check(_lib.load().uniir_layernorm_bwd(_p(x), x_stride, _p(gamma), _p(dy), int(dy.dtype == torch.float32),
                                          _p(dres), _p(dx), dx_stride, _p(dx_bf16), _p(dgamma), _p(dbeta),
                                          _p(dx_colsum), rows, width, eps, _stream()), "layernorm_bwd")
    return dx


def attention_fwd(qkv, batch, seq, heads, causal, *, out=None, lse=None):
    """softmax(q k^T / 8 [+ causal mask]) v on the packed in_proj layout qkv [batch*seq, 3*heads*64] (bf16) -> out [batch*seq, heads*64],
    lse [batch, heads, seq] (fp32, natural log).  seq <= 512 with or without the causal mask; 513 .. 1024 tokens without it (the
    streaming kernels of csrc/attention_long.hip); anything longer, or causal above 512, is UNIIR_ESHAPE.
    An fp16 qkv (forward only, the embedding towers) runs uniir_attention_fwd_f16 with the same limits and gives an fp16 out; with
    the causal mask it is a ValueError (no per-op fp16 forward is causal; the causal fp16 text tower runs from C, csrc/tower.hip)."""
    half = _dtype16(qkv, out) == DT_F16
    if half and causal:
        raise ValueError("fp16 attention is the embedding forward of the per-op towers: no causal mask")
    if out is None:
        out = torch.empty(batch * seq, heads * 64, device=qkv.device, dtype=qkv.dtype)
    if lse is None:
        lse = torch.empty(batch, heads, seq, device=qkv.device, dtype=torch.float32)
    if half:
        check(_lib.load().uniir_attention_fwd_f16(_p(qkv), _p(out), _p(lse), None, batch, seq, heads, int(causal), _stream()),
              "attention_fwd_f16")
        return out, lse
    check(_lib.load().uniir_attention_fwd(_p(qkv), _p(out), _p(lse), batch, seq, heads, int(causal), _stream()),
          "attention_fwd")
    return out, lse


def attention_fwd_causal_f16(qkv, batch, seq, heads, *, out=None, lse=None):
    """attention_fwd with the causal mask on an fp16 qkv, seq <= 512 (uniir_attention_fwd_f16 with causal = 1, the kernel the C text
    tower runs under fp16): the per-op fp16 text tower of CLIP_FF.  A wrapper of its own, so that attention_fwd keeps refusing what
    no other per-op fp16 forward may ask for.  Returns fp16 out and fp32 lse."""
    _all_fp16("attention_fwd_causal_f16", qkv, out)
    if out is None:
        out = torch.empty(batch * seq, heads * 64, device=qkv.device, dtype=torch.float16)
    if lse is None:
        lse = torch.empty(batch, heads, seq, device=qkv.device, dtype=torch.float32)
    check(_lib.load().uniir_attention_fwd_f16(_p(qkv), _p(out), _p(lse), None, batch, seq, heads, 1, _stream()),
          "attention_fwd_f16")
    return out, lse


def attention_bwd(qkv, out, dout, lse, batch, seq, heads, causal, *, dqkv=None):
    """d loss / d qkv of attention_fwd (bf16, same layout and the same limits on seq); bitwise reproducible at every length."""
    if dqkv is None:
        dqkv = torch.empty_like(qkv)
    check(_lib.load().uniir_attention_bwd(_p(qkv), _p(out), _p(dout), _p(lse), _p(dqkv), batch, seq, heads,
                                          int(causal), _stream()), "attention_bwd")
    return dqkv


def attention_one_fwd(q, k, v, kv_ld, batch, tk, heads):
    """ONE query row per item (q dense [batch, heads*64], bf16 or fp16 by its dtype) against tk <= 1024 dense keys: k / v are views of
    rows [batch*tk] with leading dimension kv_ld, head h at column h*64 (uniir_attention_one_fwd).  Returns out [batch, heads*64] and
    lse [batch, heads]: bitwise row 0 of attention_fwd on a packed qkv whose row 0 of every item is q."""
    out = torch.empty(batch, heads * 64, device=q.device, dtype=q.dtype)
    lse = torch.empty(batch, heads, device=q.device, dtype=torch.float32)
    check(_lib.load().uniir_attention_one_fwd(_p(q), _p(k), _p(v), kv_ld, _p(out), _p(lse), batch, tk, heads,
                                              int(q.dtype == torch.float16), _stream()), "attention_one_fwd")
    return out, lse


def attention_one_bwd(q, k, v, kv_ld, out, dout, lse, dq, dq_ld, dk, dv, dkv_ld, batch, tk, heads):
    """d loss / d q, k, v of attention_one_fwd (bf16) into dq ([batch] rows, dq_ld) and dk / dv ([batch*tk] rows, dkv_ld): one pass
    over K and V in one kernel at every tk (uniir_attention_one_bwd); bitwise reproducible."""
    check(_lib.load().uniir_attention_one_bwd(_p(q), _p(k), _p(v), kv_ld, _p(out), _p(dout), _p(lse), _p(dq), dq_ld, _p(dk), _p(dv),
                                              dkv_ld, batch, tk, heads, _stream()), "attention_one_bwd")


def onequery_fwd(q, q_ld, k, v, kv_ld, batch, tk, heads, *, key_len=None, kv_row_off=None, drop_p=0.0, drop_seed=0, drop_tq=1, drop_q=0):
    """ONE query row per item (row m of q at m * q_ld, bf16) that stands for row drop_q of attention_fwd_ex with tq = drop_tq: dense
    keys [batch*tk] with an optional key_len, or packed keys (kv_row_off int32 [batch + 1]); dropout at the full call's coordinates
    (uniir_onequery_fwd).  Returns out [batch, heads*64] and lse [batch, heads]: bitwise that row of the full call."""
    out = torch.empty(batch, heads * 64, device=q.device, dtype=torch.bfloat16)
    lse = torch.empty(batch, heads, device=q.device, dtype=torch.float32)
    check(_lib.load().uniir_onequery_fwd(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), heads * 64, _p(lse), _p(key_len), _p(kv_row_off),
                                         batch, tk, heads, float(drop_p), int(drop_seed), int(drop_tq), int(drop_q), _stream()),
          "onequery_fwd")
    return out, lse


def onequery_bwd(q, q_ld, k, v, kv_ld, out, dout, lse, dq, dq_ld, dk, dv, dkv_ld, batch, tk, heads, *, key_len=None, kv_row_off=None,
                 drop_p=0.0, drop_seed=0, drop_tq=1, drop_q=0):
    """d loss / d q, k, v of onequery_fwd (out / dout dense [batch, heads*64]) into dq ([batch] rows, dq_ld) and dk / dv (the key rows,
    dkv_ld; dense keys behind key_len get exact zeros): the one-pass kernel, bitwise reproducible (uniir_onequery_bwd)."""
    check(_lib.load().uniir_onequery_bwd(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), _p(dout), heads * 64, _p(lse), _p(key_len),
                                         _p(kv_row_off), _p(dq), dq_ld, _p(dk), _p(dv), dkv_ld, batch, tk, heads, float(drop_p),
                                         int(drop_seed), int(drop_tq), int(drop_q), _stream()), "onequery_bwd")


# The most tokens whose keys the resident kernels hold in LDS: csrc/attention.h ATT_SEQ_MAX.  Above it the streaming entry points
# (`_long`, csrc/attention_long.hip) run, up to ATT_LONG_SEQ_MAX = 1024; the library refuses what neither takes.
ATT_RESIDENT_MAX = 512


def _attention_long(tq, tk, causal, kv_packed):
    """the general form goes to uniir_attention_fwd_long / _bwd_long: more than ATT_RESIDENT_MAX queries or keys, no causal mask,
    dense K / V"""
    return max(tq, tk) > ATT_RESIDENT_MAX and not causal and not kv_packed


def attention_fwd_ex(q, q_ld, k, v, kv_ld, batch, tq, tk, heads, *, key_len=None, causal=False, drop_p=0.0, drop_seed=0,
                     row_off=None, kv_packed=False, rows=None):
    """separate Q / K / V views (head h at column h*64 of rows with the given leading dimension); out [batch*tq, heads*64].
    row_off (int32 [batch + 1], with rows = its total): the query rows are PACKED (item m = rows row_off[m] .. row_off[m + 1] - 1,
    uniir_attention_fwd_rows); kv_packed: K / V are rows of the same numbering (self-attention), else dense [batch][tk].
    tq, tk <= 512; without the causal mask and with dense K / V (kv_packed false) up to 1024 each: max(tq, tk) > 512 runs
    uniir_attention_fwd_long (the streaming kernels of csrc/attention_long.hip), everything at 512 and below the calls it always
    ran.  Causal or kv_packed above 512 is UNIIR_ESHAPE.
    bf16 only: fp16 operands are refused here, before any launch -- ValueError for what an fp16 forward never takes (the causal
    mask, dropout, operands of mixed types), NotImplementedError for the rest: the fp16 general form is a wrapper of its own,
    attention_fwd_ex_f16 (uniir_attn_general_fwd_f16)."""
    if torch.float16 in (q.dtype, k.dtype, v.dtype):
        _dtype16(q, k, v)
        if causal or drop_p > 0:
            raise ValueError("fp16 attention is the embedding forward: no causal mask and no dropout in the general form")
        raise NotImplementedError("uniir_attention_fwd_ex / _rows / _long take bf16; fp16 operands go through ops.attention_fwd_ex_f16")
    nrow = batch * tq if row_off is None else int(rows)
    out = torch.empty(nrow, heads * 64, device=q.device, dtype=torch.bfloat16)
    lse = torch.empty(batch, heads, tq, device=q.device, dtype=torch.float32)
    if _attention_long(tq, tk, causal, kv_packed):
        check(_lib.load().uniir_attention_fwd_long(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), heads * 64, _p(lse), _p(row_off),
                                                   _p(key_len), batch, tq, tk, heads, float(drop_p), int(drop_seed), _stream()),
              "attention_fwd_long")
    elif row_off is None:
        check(_lib.load().uniir_attention_fwd_ex(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), heads * 64, _p(lse), _p(key_len),
                                                 batch, tq, tk, heads, int(causal), float(drop_p), int(drop_seed), _stream()),
              "attention_fwd_ex")
    else:
        if causal:
            raise ValueError("packed query rows: non-causal attention only (the causal packed form is uniir_attention_fwd_packed)")
        check(_lib.load().uniir_attention_fwd_rows(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), heads * 64, _p(lse), _p(row_off),
                                                   int(bool(kv_packed)), _p(key_len), batch, tq, tk, heads, float(drop_p),
                                                   int(drop_seed), _stream()), "attention_fwd_rows")
    return out, lse


def _all_fp16(what, *tensors):
    """the fp16 general form takes fp16 operands only: anything else is a ValueError, raised before anything is launched"""
    if _dtype16(*tensors) != DT_F16:
        raise ValueError(f"{what} takes fp16 operands, not {tensors[0].dtype} (bf16: the wrapper without _f16)")


def attention_fwd_ex_f16(q, q_ld, k, v, kv_ld, batch, tq, tk, heads, *, key_len=None, row_off=None, kv_packed=False, rows=None):
    """attention_fwd_ex on fp16 operands, forward only, without the causal mask and dropout (uniir_attn_general_fwd_f16): the same
    views, row_off / kv_packed / rows and key_len; tq, tk <= 512, with dense K / V up to 1024 each.  Returns fp16 out
    [batch*tq or rows, heads*64] and fp32 lse [batch, heads, tq]."""
    _all_fp16("attention_fwd_ex_f16", q, k, v)
    nrow = batch * tq if row_off is None else int(rows)
    out = torch.empty(nrow, heads * 64, device=q.device, dtype=torch.float16)
    lse = torch.empty(batch, heads, tq, device=q.device, dtype=torch.float32)
    check(_lib.load().uniir_attn_general_fwd_f16(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), heads * 64, _p(lse), _p(row_off),
                                                 int(bool(kv_packed)), _p(key_len), batch, tq, tk, heads, _stream()),
          "attn_general_fwd_f16")
    return out, lse


def onequery_fwd_f16(q, q_ld, k, v, kv_ld, batch, tk, heads, *, key_len=None, kv_row_off=None):
    """onequery_fwd on fp16 operands, without dropout (uniir_onequery_fwd_f16): out fp16 [batch, heads*64] and lse [batch, heads] are
    bitwise row 0 of attention_fwd_ex_f16 on the same operands."""
    _all_fp16("onequery_fwd_f16", q, k, v)
    out = torch.empty(batch, heads * 64, device=q.device, dtype=torch.float16)
    lse = torch.empty(batch, heads, device=q.device, dtype=torch.float32)
    check(_lib.load().uniir_onequery_fwd_f16(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), heads * 64, _p(lse), _p(key_len),
                                             _p(kv_row_off), batch, tk, heads, _stream()), "onequery_fwd_f16")
    return out, lse


def attention_rel_fwd_f16(qkv, rel_emb, table, batch, seq, heads, scale=1.0):
    """T5-style self-attention on an fp16 packed qkv [batch*seq, 3*heads*64], forward only and without dropout: logits = scale * q.k
    + rel_emb[table[key - query + seq - 1]][head] (rel_emb fp32 [buckets, heads], table int32 [2 seq - 1]).  Up to ATT_RESIDENT_MAX
    tokens uniir_attn_rel_fwd_f16, above it uniir_attn_rel_fwd_long_f16 (up to 1024) -- the rule of the bf16 stack
    (clipff_model._rel_entry).  Returns fp16 out [batch*seq, heads*64] and fp32 lse [batch, heads, seq]."""
    _all_fp16("attention_rel_fwd_f16", qkv)
    out = torch.empty(batch * seq, heads * 64, device=qkv.device, dtype=torch.float16)
    lse = torch.empty(batch, heads, seq, device=qkv.device, dtype=torch.float32)
    name = "uniir_attn_rel_fwd_long_f16" if seq > ATT_RESIDENT_MAX else "uniir_attn_rel_fwd_f16"
    check(getattr(_lib.load(), name)(_p(qkv), _p(out), _p(lse), _p(rel_emb), _p(table), int(rel_emb.shape[0]), float(scale), batch, seq,
                                     heads, _stream()), name[len("uniir_"):])
    return out, lse


def rmsnorm_fwd(x, gamma, eps, *, out_bf16=None, out_f32=None, rows=None, width=None, x_stride=None, dtype16=torch.bfloat16):
    """T5's RMS norm of fp32 rows, in the style of layernorm_fwd: out_bf16 is the 16-bit output; an fp16 tensor there (or dtype16 =
    torch.float16 when there is none: this function allocates it, or the call has the fp32 output alone) takes
    uniir_rmsnorm_fwd_f16 -- the same fp32 result, rounded to fp16"""
    width = width or x.shape[-1]
    rows = rows if rows is not None else x.numel() // width
    x_stride = x_stride or width
    if out_bf16 is None and out_f32 is None:
        out_bf16 = torch.empty(rows, width, device=x.device, dtype=dtype16)
    if (out_bf16.dtype if out_bf16 is not None else dtype16) == torch.float16:
        check(_lib.load().uniir_rmsnorm_fwd_f16(_p(x), x_stride, _p(gamma), _p(out_bf16), _p(out_f32), rows, width, eps, _stream()),
              "rmsnorm_fwd_f16")
        return out_bf16 if out_bf16 is not None else out_f32
    check(_lib.load().uniir_rmsnorm_fwd(_p(x), x_stride, _p(gamma), _p(out_bf16), _p(out_f32), rows, width, eps, _stream()),
          "rmsnorm_fwd")
    return out_bf16 if out_bf16 is not None else out_f32


def attention_bwd_ex(q, q_ld, k, v, kv_ld, out, dout, lse, dq, dq_ld, dk, dv, dkv_ld, batch, tq, tk, heads, *,
                     key_len=None, causal=False, drop_p=0.0, drop_seed=0, row_off=None, kv_packed=False):
    """d loss / d q, k, v of attention_fwd_ex into dq / dk / dv (same arguments, same limits, the same choice of entry point)"""
    if _attention_long(tq, tk, causal, kv_packed):
        check(_lib.load().uniir_attention_bwd_long(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), _p(dout), heads * 64, _p(lse),
                                                   _p(row_off), _p(key_len), _p(dq), dq_ld, _p(dk), _p(dv), dkv_ld, batch, tq, tk,
                                                   heads, float(drop_p), int(drop_seed), _stream()), "attention_bwd_long")
    elif row_off is None:
        check(_lib.load().uniir_attention_bwd_ex(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), _p(dout), heads * 64, _p(lse),
                                                 _p(key_len), _p(dq), dq_ld, _p(dk), _p(dv), dkv_ld, batch, tq, tk, heads,
                                                 int(causal), float(drop_p), int(drop_seed), _stream()), "attention_bwd_ex")
    else:
        check(_lib.load().uniir_attention_bwd_rows(_p(q), q_ld, _p(k), _p(v), kv_ld, _p(out), _p(dout), heads * 64, _p(lse),
                                                   _p(row_off), int(bool(kv_packed)), _p(key_len), _p(dq), dq_ld, _p(dk), _p(dv),
                                                   dkv_ld, batch, tq, tk, heads, float(drop_p), int(drop_seed), _stream()),
              "attention_bwd_rows")


class DropSeeds:
    """Seeds of the counter-based dropout masks of one forward pass (csrc/common.h drop_hash): one draw from torch's CPU
    generator per forward (torch.manual_seed pins the masks), one derived 32-bit seed per dropout site; backward reuses
    the seeds kept in the activation stash."""

    def __init__(self):
        self.base = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())
        self.n = 0

    def next(self):
        self.n += 1
        return (self.base + self.n * 0x9E3779B1) & 0xFFFFFFFF


def dropout_f32(x, p, seed, *, resid=None, out_f32=None, out_bf16=None, rowscale=None, rows_per_scale=0, row_map=None):
    """(resid +) x * mask [* rowscale[row // rows_per_scale]] of an fp32 [rows, cols] tensor -> fp32 and / or bf16.
    row_map (int32 [rows]): x holds PACKED rows, row r being row row_map[r] of the logical tensor the mask is defined on"""
    rows, cols = x.shape
    if row_map is not None:
        check(_lib.load().uniir_dropout_f32_rows(_p(x), _p(resid), _p(out_f32), _p(out_bf16), rows, cols, float(p), int(seed),
                                                 _p(row_map), _stream()), "dropout_f32_rows")
        return
    check(_lib.load().uniir_dropout_f32(_p(x), _p(resid), _p(out_f32), _p(out_bf16), rows, cols, float(p), int(seed),
                                        _p(rowscale), int(rows_per_scale), _stream()), "dropout_f32")


def dropout_bf16_(x, p, seed, *, rowscale=None, rows_per_scale=0, row_map=None):
    """in place x *= mask [* rowscale[row // rows_per_scale]] of a contiguous bf16 [rows, cols] gradient (row_map: see dropout_f32)"""
    rows, cols = x.shape
    if row_map is not None:
        check(_lib.load().uniir_dropout_bf16_rows(_p(x), _p(x), rows, cols, cols, float(p), int(seed), _p(row_map), _stream()),
              "dropout_bf16_rows")
        return
    check(_lib.load().uniir_dropout_bf16(_p(x), _p(x), rows, cols, cols, float(p), int(seed), _p(rowscale),
                                         int(rows_per_scale), _stream()), "dropout_bf16")


def grad_guard_chunk():
    """elements per partial sum of the gradient guard (a compile-time constant of the library)"""
    return int(_lib.load().uniir_grad_guard_chunk())


class GradGuardPlan:
    """the host arrays of one uniir_grad_guard call over fixed ranges: [(flat fp32 tensor, lo, hi)] -> pointers, counts and the
    workspace size; built once per layout, launched every step (launch())"""

    def __init__(self, ranges):
        n = len(ranges)
        self.key = tuple((t.data_ptr(), lo, hi) for t, lo, hi in ranges)
        self.ptrs = (C.c_void_p * max(1, n))(*[t.data_ptr() + 4 * lo for t, lo, _ in ranges])
        self.counts = (C.c_int64 * max(1, n))(*[hi - lo for _, lo, hi in ranges])
        self.n = n
        self.workspace_bytes = int(_lib.load().uniir_grad_guard_workspace_bytes(self.counts, n))
        if self.workspace_bytes < 0:
            raise RuntimeError("uniir_grad_guard: ranges refused (a count below 0 or of 2^40 elements and more)")

    def launch(self, grad_scale, max_norm, skip_nonfinite, ctl, workspace):
        check(_lib.load().uniir_grad_guard(self.ptrs, self.counts, self.n, float(grad_scale), float(max_norm), int(skip_nonfinite),
                                           _p(ctl), _p(workspace), workspace.numel() if workspace is not None else 0, _stream()),
              "grad_guard")


def call(name, *args):
    """Generic checked call: tensors are converted to device pointers, the stream is appended."""
    conv = [(_p(a) if isinstance(a, torch.Tensor) else a) for a in args]
    check(getattr(_lib.load(), name)(*conv, _stream()), name)
