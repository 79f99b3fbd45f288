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

    def __init__(self, store, names, dtype16=torch.bfloat16):
        self.st, self.names = store, names
        self.half = dtype16 == torch.float16          # the 16-bit weights come from the store's fp16 shadow

    def w16(self, k):
        return self.st.w16h(self.names[k]) if self.half else self.st.w16(self.names[k])

    def p(self, k):
        return self.st.p(self.names[k])

    def g(self, k):
        return self.st.grad_view(self.names[k])


def block_set_bytes(R, W, heads):
    """bytes of one block's rebuilt set (what block_sublayers writes for the backward) at R rows of width W: qkv 6W, ao 2W, x2 4W,
    f 8W, h1 2W, h2 2W per row and lse 4 * heads per row.  A stored block keeps this set plus its fp32 input (4W per row); a
    recomputed block keeps the input alone, and ONE set exists at a time."""
    return R * (24 * W + 4 * heads)


def _block_set(R, W, M, T, heads, dev):
    """fresh buffers of one block's set, in the order of a stash entry after its input: qkv, ao, lse, x2, f, h1, h2"""
    bf = dict(device=dev, dtype=torch.bfloat16)
    return (torch.empty(R, 3 * W, **bf), torch.empty(R, W, **bf), torch.empty(M, heads, T, device=dev, dtype=torch.float32),
            torch.empty(R, W, device=dev, dtype=torch.float32), torch.empty(R, 4 * W, **bf), torch.empty(R, W, **bf),
            torch.empty(R, W, **bf))


def block_sublayers(b, x, bufs, g, M, T, W, heads, causal, eps, act, row_scale):
    """Block `b` (_Blk) from the fp32 residual stream x that enters it up to the MLP's c_fc: ln_1, in_proj, attention, out_proj +
    residual (row_scale: the DropPath factors per row of that branch, or None), ln_2, c_fc + activation -- everything of the block
    that its backward reads, written into bufs = (qkv, ao, lse, x2, f, h1, h2); act(f) goes to g.  The per-op twin of
    block_fwd_sublayers in csrc/tower.hip: the stored forward, the recompute forward and the rebuild in tower_bwd call THIS function
    with the same arguments -- same kernels, same shapes, same operand values, deterministic kernels -> the same bits.  The block's
    c_proj GEMM is not part of it: no backward reads a block's output.
    f None (forward-only pass): the pre-activation is not needed, only act(f) is written (EPI_ACT_ONLY).
    The 16-bit type is that of the buffers and of b's weights (_Blk's dtype16): every op follows its operands (ops.linear_fwd,
    ops.layernorm_fwd, ops.attention_fwd), so fp16 buffers with an fp16 _Blk run the fp16 forward."""
    qkv, ao, lse, x2, f, h1, h2 = bufs
    R = M * T
    ops.layernorm_fwd(x, b.p("ln1w"), b.p("ln1b"), eps, out_bf16=h1, rows=R, width=W)
    ops.linear_fwd(h1, b.w16("wqkv"), b.p("bqkv"), out=qkv)
    if causal and qkv.dtype == torch.float16:      # CLIP_FF's text tower under fp16: the causal fp16 forward has a wrapper of its own
        ao, lse = ops.attention_fwd_causal_f16(qkv, M, T, heads, out=ao, lse=lse)
    else:
        ao, lse = ops.attention_fwd(qkv, M, T, heads, causal, out=ao, lse=lse)      # (a forward-only pass passes None: fresh ones)
    ops.linear_fwd(ao, b.w16("wo"), b.p("bo"), out=x2, epilogue=ops.EPI_RESID_F32, resid=x, row_scale=row_scale)
    ops.layernorm_fwd(x2, b.p("ln2w"), b.p("ln2b"), eps, out_bf16=h2, rows=R, width=W)
    if f is not None:
        ops.linear_fwd(h2, b.w16("wfc"), b.p("bfc"), out=f, epilogue=ops.EPI_BIAS_ACT, C2=g, act=act)
    else:
        ops.linear_fwd(h2, b.w16("wfc"), b.p("bfc"), out=g, epilogue=ops.EPI_ACT_ONLY, act=act)


def tower_fwd(st, names, layers, x, M, T, W, heads, causal, save, eps=1e-5, act=ops.ACT_QUICKGELU, rowscale=None,
              recompute_from=None, dtype16=torch.bfloat16):
    """pre-LN residual blocks (CLIP resblocks; with eps / act / names overridden also the BLIP ViT blocks).
    rowscale fp32 [layers, 2, M]: DropPath factors (0 or 1/keep per item) of the two residual branches of each block
    (BLIP ViT-large in train mode, backbone/vit.py:79-80); None = no DropPath (the residual add stays in the GEMM).
    recompute_from (with save): blocks i >= recompute_from keep only their fp32 input -- their stash entry is (x,) -- and run their
    sublayers into one set of buffers they all share; tower_bwd rebuilds the set from x right before such a block's backward.
    Blocks below the boundary are stored whole.  None, or any value >= layers: every block is stored.
    dtype16 = torch.float16 (forward only, save False): 16-bit activations in fp16, weights from the store's fp16 shadow; the residual
    stream, LayerNorm statistics and accumulation stay fp32.  There is no fp16 backward: with save it raises."""
    if dtype16 not in (torch.bfloat16, torch.float16):
        raise ValueError(f"dtype16 is torch.bfloat16 or torch.float16, not {dtype16!r}")
    if save and dtype16 == torch.float16:
        raise RuntimeError("the fp16 tower forward keeps nothing for a backward (save=True needs dtype16=torch.bfloat16)")
    R = M * T
    dev = x.device
    h = torch.empty(R, W, device=dev, dtype=dtype16)
    g = torch.empty(R, 4 * W, device=dev, dtype=dtype16)
    saved = []
    # DropPath factors per ROW (item factor repeated over its T tokens): applied inside the residual GEMM's epilogue
    rs_rows = None if rowscale is None else rowscale.repeat_interleave(T, dim=2).contiguous()
    first_rc = layers if (recompute_from is None or not save) else max(int(recompute_from), 0)
    shared = None        # the one set of the recomputed blocks
    for i in range(layers):
        b = _Blk(st, names(i), dtype16)
        if not save:      # forward only: both LayerNorm outputs pass through h, no pre-activation f
            bufs = (torch.empty(R, 3 * W, device=dev, dtype=dtype16), None, None,
                    torch.empty(R, W, device=dev, dtype=torch.float32), None, h, h)
        elif i >= first_rc:
            if shared is None:
                shared = _block_set(R, W, M, T, heads, dev)
            bufs = shared
        else:
            # a stored block keeps the two LayerNorm outputs too, for the weight gradients (26 GB at ViT-L/14 x 1024 items:
            # cheaper than re-reading the fp32 stream to recompute them in backward)
            bufs = _block_set(R, W, M, T, heads, dev)
        block_sublayers(b, x, bufs, g, M, T, W, heads, causal, eps, act, None if rs_rows is None else rs_rows[i, 0])
        xn = ops.linear_fwd(g, b.w16("wproj"), b.p("bproj"), epilogue=ops.EPI_RESID_F32, resid=bufs[3],
                            row_scale=None if rs_rows is None else rs_rows[i, 1])
        if save:
            saved.append((x,) if i >= first_rc else (x,) + bufs)
        x = xn
        del bufs, xn        # (a forward-only pass: the block's buffers go back before the next block takes its own)
    return x, saved


def tower_bwd(st, names, layers, dx, dxb, saved, M, T, W, heads, causal, eps=1e-5, act=ops.ACT_QUICKGELU, rowscale=None,
              block_done=None):
    """dx fp32 [R,W] and its bf16 copy dxb: gradient w.r.t. the tower output.  Returns d(tower input) (fp32).
    With DropPath factors (rowscale, see tower_fwd) the gradient entering a branch is rowscale * dx: the LayerNorm backward
    that produces dx writes its bf16 copy and the branch's bias gradient already scaled (uniir_layernorm_bwd_ex); only the
    tower's incoming gradient is scaled by a separate pass.  block_done(i), if given, is called once block i's parameter
    gradients are complete (DDP overlap: CLIP.block_done hands them to the gradient reducer).
    A block whose stash entry holds only its input (tower_fwd's recompute_from) is rebuilt first: block_sublayers on the stored x,
    with the forward's arguments (the same rowscale tensor: no second random draw), into one set allocated once per call.  The
    rebuild writes that set and g -- c_fc's epilogue needs somewhere to put act(f), and g is dead between blocks: the dgrad below
    fills it again -- never the gradients that are live across blocks (dx, dx2, dxb, df, dh)."""
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
    shared = None        # the one set the recomputed blocks are rebuilt into
    for i in reversed(range(layers)):
        b = _Blk(st, names(i))
        entry = saved[i]
        saved[i] = None
        if len(entry) == 1:
            if shared is None:
                shared = _block_set(R, W, M, T, heads, dev)
            x = entry[0]
            block_sublayers(b, x, shared, g, M, T, W, heads, causal, eps, act, None if rs_rows is None else rs_rows[i, 0])
            qkv, ao, lse, x2, f, h1, h2 = shared
        else:
            x, qkv, ao, lse, x2, f, h1, h2 = entry
            shared = None        # the blocks below the boundary are all stored: the set is not needed again
        del entry
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
