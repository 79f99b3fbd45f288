"""The fp32 launch layer (precision = "fp32", precision.py): what every fp32 embedding forward is written on.  Every GEMM is the
exact-fp32 MFMA uniir_sgemm on the fp32 masters of a store (no shadow is read or built), with uniir_bias_act_f32 for bias /
activation / residual, the fp32 outputs of the LayerNorm and RMS norm kernels and uniir_attention_f32_fwd (csrc/fp32_path.hip).
Forward only: every output is a fresh buffer, nothing is kept.  The primitives, the patch stem and the pre-LN block body of the CLIP
towers and the BLIP ViT are here; the BERT layer, the T5 layer, the poolers and the fusions stay with their models.  It shares
nothing with the dtype16 path of resblocks.py, which runs other kernels (fused epilogues), but reads the same role tables."""
import torch

from . import ops


def linear_f32(x, w, bias=None, *, act=-1, resid=None, w_kn=False):
    """y[M,N] = act(x[M,K] @ w[N,K]^T + bias) (+ resid), all fp32; w_kn: w is [K,N] (a CLIP projection), y = x @ w"""
    M, K = x.shape
    N = w.shape[1] if w_kn else w.shape[0]
    y = torch.empty(M, N, device=x.device, dtype=torch.float32)
    ops.call("uniir_sgemm", x, K, 1, w, *((N, 1) if w_kn else (1, K)), y, N, M, N, K, 1.0)
    if bias is not None or resid is not None or act >= 0:
        ops.call("uniir_bias_act_f32", y, bias, resid, M, N, act)
    return y


def layernorm_f32(x, w, b, eps=1e-5):
    y = torch.empty_like(x)
    ops.layernorm_fwd(x, w, b, eps, out_f32=y, rows=x.shape[0], width=x.shape[1])
    return y


def rmsnorm_f32(x, w, eps):
    R, D = x.shape
    y = torch.empty_like(x)
    ops.call("uniir_rmsnorm_fwd", x, D, w, None, y, R, D, eps)
    return y


def attention_f32(q, q_ld, k, v, kv_ld, key_len, M, tq, tk, heads, causal=False):
    """softmax(q k^T / 8 [+ causal mask]) v on separate views (head h at column h*64); key_len int32 [M] or None -> [M*tq, heads*64]"""
    out = torch.empty(M * tq, heads * 64, device=q.device, dtype=torch.float32)
    ops.call("uniir_attention_f32_fwd", q, q_ld, k, v, kv_ld, out, heads * 64, key_len, M, tq, tk, heads, int(causal), 0.125)
    return out


def patch_tokens_f32(images, P, w, bias, cls, pos):
    """the patch stem: images [M,3,res,res], w [W,3,P,P] -> fp32 [M*T, W] = class token | patch projections, + pos; and T"""
    M, g, W = images.shape[0], images.shape[-1] // P, w.shape[0]
    T = g * g + 1
    # im2col is a pure permutation (no arithmetic): [M,3,g,P,g,P] -> [M*g*g, 3*P*P], the order w.view(W,-1) has
    patches = images.float().contiguous().view(M, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(M * g * g, 3 * P * P).contiguous()
    po = linear_f32(patches, w.view(W, 3 * P * P), bias)
    x = torch.empty(M * T, W, device=images.device, dtype=torch.float32)
    ops.call("uniir_vit_assemble_f32", po, cls, pos, x, M, T, W)
    return x, T


def tower_fwd_f32(p, names, layers, x, M, T, W, heads, causal, eps=1e-5, act=ops.ACT_QUICKGELU):
    """resblocks.tower_fwd's pre-LN blocks in fp32: p(name) is the store's fp32 view, names(i) block i's role table"""
    for i in range(layers):
        n = names(i)
        h = layernorm_f32(x, p(n["ln1w"]), p(n["ln1b"]), eps)
        qkv = linear_f32(h, p(n["wqkv"]), p(n["bqkv"]))
        ao = attention_f32(qkv, 3 * W, qkv[:, W:], qkv[:, 2 * W:], 3 * W, None, M, T, T, heads, causal)
        x = linear_f32(ao, p(n["wo"]), p(n["bo"]), resid=x)
        h = layernorm_f32(x, p(n["ln2w"]), p(n["ln2b"]), eps)
        g = linear_f32(h, p(n["wfc"]), p(n["bfc"]), act=act)
        x = linear_f32(g, p(n["wproj"]), p(n["bproj"]), resid=x)
    return x
