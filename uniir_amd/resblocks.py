"""Pre-LN residual blocks as per-op launch sequences over a FlatStore: the CLIP towers without pooling of CLIP_FF and the BLIP ViT.
(CLIP_SF's pooled towers run the same block sequence from C in one call, csrc/tower.hip.)  A tower reads block i's tensors through
names(i), a table from the roles wqkv, bqkv, wo, bo, ln1w, ln1b, wfc, bfc, wproj, bproj, ln2w, ln2b to tensor names of the store."""
import torch

from . import ops


def clip_block_names(prefix, i):
    """the name table of CLIP residual block i of the tower `prefix` ("visual.transformer" / "transformer")"""
    p = f"{prefix}.resblocks.{i}"
    return dict(wqkv=f"{p}.attn.in_proj_weight", bqkv=f"{p}.attn.in_proj_bias", wo=f"{p}.attn.out_proj.weight",
                bo=f"{p}.attn.out_proj.bias", ln1w=f"{p}.ln_1.weight", ln1b=f"{p}.ln_1.bias", wfc=f"{p}.mlp.c_fc.weight",
                bfc=f"{p}.mlp.c_fc.bias", wproj=f"{p}.mlp.c_proj.weight", bproj=f"{p}.mlp.c_proj.bias", ln2w=f"{p}.ln_2.weight",
                ln2b=f"{p}.ln_2.bias")


class _Blk:
    """one residual block's tensors inside a FlatStore"""

    def __init__(self, store, names):
        self.st, self.names = store, names

    def w16(self, k):
        return self.st.w16(self.names[k])

    def p(self, k):
        return self.st.p(self.names[k])

    def g(self, k):
        return self.st.grad_view(self.names[k])


def tower_fwd(st, names, layers, x, M, T, W, heads, causal, save, eps=1e-5, act=ops.ACT_QUICKGELU, rowscale=None):
    """pre-LN residual blocks (CLIP resblocks; with eps / act / names overridden also the BLIP ViT blocks).
    rowscale fp32 [layers, 2, M]: DropPath factors (0 or 1/keep per item) of the two residual branches of each block
    (BLIP ViT-large in train mode, backbone/vit.py:79-80); None = no DropPath (the residual add stays in the GEMM)"""
    R = M * T
    dev = x.device
    h = torch.empty(R, W, device=dev, dtype=torch.bfloat16)
    g = torch.empty(R, 4 * W, device=dev, dtype=torch.bfloat16)
    saved = []
    # DropPath factors per ROW (item factor repeated over its T tokens): applied inside the residual GEMM's epilogue
    rs_rows = None if rowscale is None else rowscale.repeat_interleave(T, dim=2).contiguous()
    for i in range(layers):
        b = _Blk(st, names(i))
        # with save, the two LayerNorm outputs are kept for the weight gradients (26 GB at ViT-L/14 x 1024 items:
        # cheaper than re-reading the fp32 stream to recompute them in backward)
        h1 = torch.empty(R, W, device=dev, dtype=torch.bfloat16) if save else h
        ops.layernorm_fwd(x, b.p("ln1w"), b.p("ln1b"), eps, out_bf16=h1, rows=R, width=W)
        qkv = ops.linear_fwd(h1, b.w16("wqkv"), b.p("bqkv"))
        ao, lse = ops.attention_fwd(qkv, M, T, heads, causal)
        if rowscale is None:
            x2 = ops.linear_fwd(ao, b.w16("wo"), b.p("bo"), epilogue=ops.EPI_RESID_F32, resid=x)
        else:
            x2 = ops.linear_fwd(ao, b.w16("wo"), b.p("bo"), epilogue=ops.EPI_RESID_F32, resid=x, row_scale=rs_rows[i, 0])
        h2 = torch.empty(R, W, device=dev, dtype=torch.bfloat16) if save else h
        ops.layernorm_fwd(x2, b.p("ln2w"), b.p("ln2b"), eps, out_bf16=h2, rows=R, width=W)
        if save:
            f = torch.empty(R, 4 * W, device=dev, dtype=torch.bfloat16)
            ops.linear_fwd(h2, b.w16("wfc"), b.p("bfc"), out=f, epilogue=ops.EPI_BIAS_ACT, C2=g, act=act)
        else:       # forward only: the pre-activation is not needed, only act(f) is written
            f = None
            ops.linear_fwd(h2, b.w16("wfc"), b.p("bfc"), out=g, epilogue=ops.EPI_ACT_ONLY, act=act)
        if rowscale is None:
            xn = ops.linear_fwd(g, b.w16("wproj"), b.p("bproj"), epilogue=ops.EPI_RESID_F32, resid=x2)
        else:
            xn = ops.linear_fwd(g, b.w16("wproj"), b.p("bproj"), epilogue=ops.EPI_RESID_F32, resid=x2, row_scale=rs_rows[i, 1])
        if save:
            saved.append((x, qkv, ao, lse, x2, f, h1, h2))
        x = xn
    return x, saved


def tower_bwd(st, names, layers, dx, dxb, saved, M, T, W, heads, causal, eps=1e-5, act=ops.ACT_QUICKGELU, rowscale=None,
              block_done=None):
    """dx fp32 [R,W] and its bf16 copy dxb: gradient w.r.t. the tower output.  Returns d(tower input) (fp32).
    With DropPath factors (rowscale, see tower_fwd) the gradient entering a branch is rowscale * dx: the LayerNorm backward
    that produces dx writes its bf16 copy and the branch's bias gradient already scaled (uniir_layernorm_bwd_ex); only the
    tower's incoming gradient is scaled by a separate pass.  block_done(i), if given, is called once block i's parameter
    gradients are complete (DDP overlap: CLIP.block_done hands them to the gradient reducer)."""
    R = M * T
    dev = dx.device
    g = torch.empty(R, 4 * W, device=dev, dtype=torch.bfloat16)
    df = torch.empty(R, 4 * W, device=dev, dtype=torch.bfloat16)
    dh = torch.empty(R, W, device=dev, dtype=torch.bfloat16)
    # bias gradient of the last block's c_proj: column sums of the incoming gradient (the other blocks get theirs from
    # the LayerNorm backward that produces their incoming gradient)
    rs_rows = None if rowscale is None else rowscale.repeat_interleave(T, dim=2).contiguous()     # factor per row
    if rowscale is not None:
        ops.dropout_bf16_(dxb, 0.0, 0, rowscale=rowscale[layers - 1, 1], rows_per_scale=T)
    ops.call("uniir_colsum_bf16", dxb, W, _Blk(st, names(layers - 1)).g("bproj"), R, W)
    for i in reversed(range(layers)):
        b = _Blk(st, names(i))
        x, qkv, ao, lse, x2, f, h1, h2 = saved[i]
        saved[i] = None
        # d(mlp): df = (dx @ Wproj) * act'(f); the same epilogue re-materialises g = act(f) for dWproj and sums
        # df's columns into the c_fc bias gradient
        ops.linear_dgrad(dxb, b.w16("wproj"), out=df, aux=f, act_out=g, colsum=b.g("bfc"), act=act)
        ops.linear_wgrad(dxb, g, b.g("wproj"))
        ops.linear_wgrad(df, h2, b.g("wfc"))
        ops.linear_dgrad(df, b.w16("wfc"), out=dh)                               # dh := d ln_2 out
        dx2 = torch.empty(R, W, device=dev, dtype=torch.float32)
        ops.layernorm_bwd(x2, b.p("ln2w"), dh, b.g("ln2w"), b.g("ln2b"), eps, dres=dx, dx=dx2, dx_bf16=dxb,
                          rows=R, width=W, dx_colsum=b.g("bo"),             # d x2 also is d(out_proj out): its bias grad
                          branch_scale=None if rs_rows is None else rs_rows[i, 0])
        del x2, f, h2
        ops.linear_wgrad(dxb, ao, b.g("wo"))
        ops.linear_dgrad(dxb, b.w16("wo"), out=dh)                               # dh := d attn out
        dqkv = ops.attention_bwd(qkv, ao, dh, lse, M, T, heads, causal)
        del qkv, ao, lse
        ops.linear_wgrad(dqkv, h1, b.g("wqkv"), dbias=b.g("bqkv"))             # + the in_proj bias gradient, same pass over dqkv
        ops.linear_dgrad(dqkv, b.w16("wqkv"), out=dh)                            # dh := d ln_1 out
        del dqkv, h1
        ops.layernorm_bwd(x, b.p("ln1w"), dh, b.g("ln1w"), b.g("ln1b"), eps, dres=dx2, dx=dx, dx_bf16=dxb,
                          rows=R, width=W, dx_colsum=(_Blk(st, names(i - 1)).g("bproj") if i > 0 else None),
                          branch_scale=None if (rs_rows is None or i == 0) else rs_rows[i - 1, 1])
        del x, dx2
        if block_done is not None:
            block_done(i)
    return dx
