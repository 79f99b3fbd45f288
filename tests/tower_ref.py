"""Stage references of the CLIP tower calls (csrc/tower.hip): one function per launch of tower_fwd, tower_bwd_head, tower_bwd_blocks
(the general block and last_block_bwd_pooled) and tower_bwd_stem, each judged from the inputs that launch had.

Not a test module and free of any GPU call.  tests/test_tower_stages_gpu.py reads the device's intermediates out of the caller's
workspace (uniir_clip_tower_layout), puts them into a TRACE -- a dict name -> tensor -- and calls verify(); tests/test_tower_ref.py
builds a trace on the CPU with compose() and checks the references' own wiring against the autograd of oracle.clip_oracle, and that
verify() flags every seeded wiring defect of MUTATIONS.

There is no arithmetic model here.  A stage is a call of gemm_ref.gemm_reference, attention_ref.forward_reference /
backward_reference, fp32_ref.norm_fwd / norm_bwd or a glue_ref function on tensors taken from the trace, and returns what those
return: (reference, bound) in float64, or a bit-exact expectation (bound None) for pure data movement and single fp32 operations.
Whatever composes them -- which tensor feeds which launch, which rows, which column range of qkv / wqkv / bqkv, which gradient
buffer a sum lands in -- is stated here once, independently of tower.hip, and that is what the tests judge.

Trace names.  Forward: input, patches, po, x0, eot; per layer i: x.i (the stream ENTERING block i; x.L leaves the last block), h1.i,
qkv.i, ao.i, lse.i, x2.i, h2.i, f.i, g.i; the pooled last block's pl_h1, pl_q, pl_ao, pl_lse, pl_x, pl_x2, pl_h2, pl_f, pl_g; rows
(the pooled row of every item), pooled, emb.  Backward: demb, demb16, dpooled, drows, dx.i / dxb.i (the gradient of x.i: dx.L leaves
the head, dx.0 enters the stem), df.i, dx2.i, dqkv.i, dh.i (d ln_1 out, the last value the buffer holds), pl_dxb.h (after the head),
pl_df, pl_dx2, pl_dxb, pl_dh, pl_dqkv, pl_dhq, dx0, dpo, dconv.  Parameter gradients: g0.<param> the contents before the backward
(the contract is +=), g.<param> after it; <param> is b<i>.<name> for a block and conv, cls, pos, ln_pre_w, ln_pre_b, tok, ln_post_w,
ln_post_b, proj for the tower.

Two-stage checks.  Three results have an input that the same call overwrites: dx2 / g_ln2 / g_bo (d ln_2 out), dqkv (d attention
out), and the pooled block's pl_dx2.  The lost intermediate is rebuilt by its GEMM reference from tensors that survive (df; bf16(dx2),
which is bit for bit what ln_2's backward left in dxb); the operator behind it is linear in that intermediate, so the bound is the
stage's own plus the operator with absolute coefficients applied to the intermediate's bound (fp32_ref.norm_bwd_dy_sensitivity,
attention_ref.backward_dout_sensitivity).

Masks.  A stage that defines only part of a tensor (the K | V columns of the pooled block's qkv, the Q rows of its g_wqkv, the rows
of dh that are not pooled) says which; compose() merges the parts, verify() judges each part against its own stage.
"""
import math
from dataclasses import dataclass

import torch

import attention_ref as A
import fp32_ref as F
import gemm_ref as Gm
import glue_cases as GC
import glue_ref as G

BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
EPS = 1e-5
SCALE = 0.125
ATT_SEQ_MAX = 512                 # csrc/attention.h: a head's keys resident in LDS; pool_last_block = 1 pools up to here
BLOCK_PARAMS = ("ln1_w", "ln1_b", "ln2_w", "ln2_b", "wqkv", "bqkv", "wo", "bo", "wfc", "bfc", "wproj", "bproj")


@dataclass
class Spec:
    name: str
    is_text: bool
    W: int
    L: int
    T: int
    E: int
    M: int
    res: int = 0
    patch: int = 0
    kpad: int = 0
    vocab: int = 0
    pool: int = 0                 # uniir_clip_tower.pool_last_block
    lens: tuple = None            # packed text: the live length of every item (EOT position + 1)
    scratch: str = "on"           # whether the stream has a reduction scratch (fixed-order sums) -- glue_cases' forms

    @property
    def H(self):
        return self.W // 64

    @property
    def G(self):
        return self.T - 1

    @property
    def R(self):
        return sum(self.lens) if self.lens else self.M * self.T

    @property
    def pooled(self):
        return self.pool != 0 and (self.T <= ATT_SEQ_MAX or self.pool == 2)

    def items(self):
        """(first row, rows) of every item in the residual stream"""
        if self.lens:
            off, out = 0, []
            for n in self.lens:
                out.append((off, n))
                off += n
            return out
        return [(m * self.T, self.T) for m in range(self.M)]

    def tower_params(self):
        return ("tok", "pos", "ln_post_w", "ln_post_b", "proj") if self.is_text else \
            ("conv", "cls", "pos", "ln_pre_w", "ln_pre_b", "ln_post_w", "ln_post_b", "proj")

    def params(self):
        return [f"b{i}.{n}" for i in range(self.L) for n in BLOCK_PARAMS] + list(self.tower_params())


@dataclass
class Out:
    ref: torch.Tensor
    bound: object                 # float64 tensor, or None: the stored value is ref.to(dt) bit for bit
    dt: torch.dtype               # what the device stores
    mask: object = None           # bool, same shape: the elements this stage defines (None: all)


def gemm_tile(M, N, K, wgrad=False):
    """the kernel family uniir_gemm gives a problem (csrc/gemm.hip, restated in tests/test_gemm_paths_gpu.py): 128 x 128 tiles when
    K % 64, M < 256 or N < 128, else 256 x 256 -- and a weight gradient (ATOMIC_F32, both operands T-major) with K % 64 and
    K >= 1024 runs its multiple of 64 on the 256-tile kernel and the tail on the other (the head + tail form)"""
    if M < 256 or N < 128:
        return 128
    if K % 64:
        return 256 if wgrad and K >= 1024 else 128
    return 256


def attention_family(sp):
    """the attention kernels a tower's full blocks run, by token count (csrc/attention.hip attention_fwd_impl): the text forms hold a
    head in LDS; vision: resident up to 192 tokens, the pair-tile backward from 193 to 288, resident again to 512, streaming above"""
    if sp.is_text:
        return "causal-packed" if sp.lens else "causal"
    if sp.T > ATT_SEQ_MAX:
        return "streaming"
    return "pair-tile-bwd" if 193 <= sp.T <= 288 else "resident"


def r16(t):
    """the bf16 copy of an fp32 tensor (float64: the unrounded composition, left alone)"""
    return t if t.dtype == torch.float64 else t.to(BF16)


def _mm(a, b, **kw):
    return Gm.gemm_reference(a.double(), b.double(), **kw)


def _full(ref, bound, shape, sel, dt, device):
    """a part (ref, bound) of a larger tensor: embedded at `sel`, with the mask of that part"""
    r = torch.zeros(shape, dtype=torch.float64, device=device)
    b = torch.zeros(shape, dtype=torch.float64, device=device) if bound is not None else None
    m = torch.zeros(shape, dtype=torch.bool, device=device)
    r[sel] = ref.double() if bound is not None else ref.to(r.dtype)
    if b is not None:
        b[sel] = bound
    m[sel] = True
    return Out(r if bound is not None else _as(ref, r, sel), b, dt, m)


def _as(part, like, sel):
    """exact parts keep their own dtype (bit patterns must survive): a zero tensor of that dtype with the part embedded"""
    t = torch.zeros(like.shape, dtype=part.dtype, device=like.device)
    t[sel] = part
    return t


def _pool_rows(sp, tr):
    """absolute row of every item's pooled row (class token / EOT row)"""
    dev = tr["input"].device
    if not sp.is_text:
        return torch.arange(sp.M, device=dev) * sp.T
    eot = tr["eot"].long().to(dev)
    return eot if sp.lens else torch.arange(sp.M, device=dev) * sp.T + eot


def _klen(sp, tr, m):
    """keys the pooled row of item m attends to: all of a vision item, tokens 0 .. EOT of a caption"""
    if not sp.is_text:
        return sp.T
    return sp.lens[m] if sp.lens else int(tr["eot"][m]) + 1


def _qkv_item(qkv, s, n, H):
    rows = qkv[s:s + n]
    W = H * 64
    return tuple(rows[:, j * W:(j + 1) * W].reshape(n, H, 64) for j in range(3))


# ===================================================================================================================== the stages
def stages(sp, backward=True):
    """[(label, fn(wt, tr) -> {trace name: Out})] in launch order.  wt: the weights -- fp32 masters under their parameter names and
    their bf16 shadows under <name>16 (the GEMM operands)"""
    W, T, M, L, H, E, R = sp.W, sp.T, sp.M, sp.L, sp.H, sp.E, sp.R
    S = []
    add = lambda label, fn: S.append((label, fn))          # noqa: E731
    dev = lambda tr: tr["input"].device                    # noqa: E731

    # ------------------------------------------------------------------------------------------------------------ forward: stem
    if not sp.is_text:
        add("patchify", lambda wt, tr: {"patches": Out(G.patchify(tr["input"], sp.patch, sp.kpad), None, BF16)})
        add("conv", lambda wt, tr: {"po": Out(*_mm(tr["patches"], wt["conv16"].t(), epilogue=Gm.EPI_BF16)["C"], BF16)})
        add("vit_assemble", lambda wt, tr: {"x0": Out(G.vit_assemble(tr["po"], wt["cls"], wt["pos"], M, T), None, F32)})
        add("ln_pre", lambda wt, tr: {"x.0": Out(*F.norm_fwd(tr["x0"], wt["ln_pre_w"], wt["ln_pre_b"], EPS)["y_f32"], F32)})
    else:
        def text_embed(wt, tr):
            if sp.lens:
                x, last = G.text_embed_packed(tr["input"], wt["tok"], wt["pos"], sp.vocab, torch.tensor(sp.lens, device=dev(tr)))
            else:
                x, last = G.text_embed(tr["input"], wt["tok"], wt["pos"], sp.vocab)
            return {"x.0": Out(x, None, F32), "eot": Out(last.to(dev(tr)), None, I32)}
        add("text_embed", text_embed)

    # ---------------------------------------------------------------------------------------------------------- forward: blocks
    def ln1(i):
        return lambda wt, tr: {f"h1.{i}": Out(*F.norm_fwd(tr[f"x.{i}"], wt[f"b{i}.ln1_w"], wt[f"b{i}.ln1_b"], EPS)["y_bf16"], BF16)}

    def in_proj(i):
        return lambda wt, tr: {f"qkv.{i}": Out(*_mm(tr[f"h1.{i}"], wt[f"b{i}.wqkv16"].t(), epilogue=Gm.EPI_BF16,
                                                    bias=wt[f"b{i}.bqkv"])["C"], BF16)}

    def attn(i):
        def fn(wt, tr):
            qkv = tr[f"qkv.{i}"]
            d = qkv.device
            o, ob = torch.zeros(R, W, dtype=torch.float64, device=d), torch.zeros(R, W, dtype=torch.float64, device=d)
            ls, lb = torch.zeros(M, H, T, dtype=torch.float64, device=d), torch.zeros(M, H, T, dtype=torch.float64, device=d)
            lm = torch.zeros(M, H, T, dtype=torch.bool, device=d)
            for m, (s, n) in enumerate(sp.items()):
                q, k, v = _qkv_item(qkv, s, n, H)
                r, _ = A.forward_reference(q, k, v, scale=SCALE, dtype=BF16, valid=A.valid_mask(n, n, causal=sp.is_text, device=d))
                o[s:s + n], ob[s:s + n] = r["out"][0].reshape(n, W), r["out"][1].reshape(n, W)
                ls[m, :, :n], lb[m, :, :n], lm[m, :, :n] = r["lse"][0], r["lse"][1], True
            return {f"ao.{i}": Out(o, ob, BF16), f"lse.{i}": Out(ls, lb, F32, lm)}
        return fn

    def out_proj(i):
        return lambda wt, tr: {f"x2.{i}": Out(*_mm(tr[f"ao.{i}"], wt[f"b{i}.wo16"].t(), epilogue=Gm.EPI_RESID_F32, bias=wt[f"b{i}.bo"],
                                                   resid=tr[f"x.{i}"])["C"], F32)}

    def ln2(i):
        return lambda wt, tr: {f"h2.{i}": Out(*F.norm_fwd(tr[f"x2.{i}"], wt[f"b{i}.ln2_w"], wt[f"b{i}.ln2_b"], EPS)["y_bf16"], BF16)}

    def c_fc(i):
        # (got_f only feeds the C2 reference, which is the next stage's)
        return lambda wt, tr: {f"f.{i}": Out(*_mm(tr[f"h2.{i}"], wt[f"b{i}.wfc16"].t(), epilogue=Gm.EPI_BIAS_ACT, bias=wt[f"b{i}.bfc"],
                                                  got_f=torch.zeros(1))["C"], BF16)}

    def c_fc_act(i):
        # act(f) of the kernel's OWN stored f (gemm_ref: BIAS_ACT's C2), so the stage is judged apart from c_fc's rounding
        def fn(wt, tr):
            r = _mm(tr[f"h2.{i}"], wt[f"b{i}.wfc16"].t(), epilogue=Gm.EPI_BIAS_ACT, bias=wt[f"b{i}.bfc"], got_f=tr[f"f.{i}"])
            return {f"g.{i}": Out(*r["C2"], BF16)}
        return fn

    def c_proj(i):
        return lambda wt, tr: {f"x.{i + 1}": Out(*_mm(tr[f"g.{i}"], wt[f"b{i}.wproj16"].t(), epilogue=Gm.EPI_RESID_F32,
                                                      bias=wt[f"b{i}.bproj"], resid=tr[f"x2.{i}"])["C"], F32)}

    for i in range(L - (1 if sp.pooled else 0)):
        for label, mk in (("ln_1", ln1), ("in_proj", in_proj), ("attention", attn), ("out_proj", out_proj), ("ln_2", ln2),
                          ("c_fc", c_fc), ("c_fc act", c_fc_act), ("c_proj", c_proj)):
            add(f"{label} [{i}]", mk(i))

    # ------------------------------------------------------------------------------------------ forward: the pooled last block
    def pooled_fwd(i):
        add(f"ln_1 [{i}]", ln1(i))

        def kv_proj(wt, tr):
            r, b = _mm(tr[f"h1.{i}"], wt[f"b{i}.wqkv16"][W:].t(), epilogue=Gm.EPI_BF16, bias=wt[f"b{i}.bqkv"][W:])["C"]
            return {f"qkv.{i}": _full(r, b, (R, 3 * W), (slice(None), slice(W, 3 * W)), BF16, r.device)}
        add(f"pooled K|V proj [{i}]", kv_proj)
        add("pooled gather h1", lambda wt, tr: {"pl_h1": Out(tr[f"h1.{i}"][_pool_rows(sp, tr)], None, BF16)})
        add("pooled Q proj", lambda wt, tr: {"pl_q": Out(*_mm(tr["pl_h1"], wt[f"b{i}.wqkv16"][:W].t(), epilogue=Gm.EPI_BF16,
                                                              bias=wt[f"b{i}.bqkv"][:W])["C"], BF16)})

        def attn_one(wt, tr):
            qkv, d = tr[f"qkv.{i}"], tr[f"qkv.{i}"].device
            o, ob = torch.zeros(M, W, dtype=torch.float64, device=d), torch.zeros(M, W, dtype=torch.float64, device=d)
            ls, lb = torch.zeros(M, H, dtype=torch.float64, device=d), torch.zeros(M, H, dtype=torch.float64, device=d)
            for m, (s, n) in enumerate(sp.items()):
                kl = _klen(sp, tr, m)
                _, k, v = _qkv_item(qkv, s, kl, H)
                r, _ = A.forward_reference(tr["pl_q"][m].reshape(1, H, 64), k, v, scale=SCALE, dtype=BF16,
                                           valid=A.valid_mask(1, kl, device=d))
                o[m], ob[m] = r["out"][0].reshape(W), r["out"][1].reshape(W)
                ls[m], lb[m] = r["lse"][0][:, 0], r["lse"][1][:, 0]
            return {"pl_ao": Out(o, ob, BF16), "pl_lse": Out(ls, lb, F32)}
        add("pooled attention", attn_one)
        add("pooled gather x", lambda wt, tr: {"pl_x": Out(tr[f"x.{i}"][_pool_rows(sp, tr)], None, F32)})
        add("pooled out_proj", lambda wt, tr: {"pl_x2": Out(*_mm(tr["pl_ao"], wt[f"b{i}.wo16"].t(), epilogue=Gm.EPI_RESID_F32,
                                                                 bias=wt[f"b{i}.bo"], resid=tr["pl_x"])["C"], F32)})
        add("pooled ln_2", lambda wt, tr: {"pl_h2": Out(*F.norm_fwd(tr["pl_x2"], wt[f"b{i}.ln2_w"], wt[f"b{i}.ln2_b"], EPS)["y_bf16"],
                                                        BF16)})
        add("pooled c_fc", lambda wt, tr: {"pl_f": Out(*_mm(tr["pl_h2"], wt[f"b{i}.wfc16"].t(), epilogue=Gm.EPI_BIAS_ACT,
                                                            bias=wt[f"b{i}.bfc"], got_f=torch.zeros(M, 4 * W))["C"], BF16)})
        add("pooled c_fc act", lambda wt, tr: {"pl_g": Out(*_mm(tr["pl_h2"], wt[f"b{i}.wfc16"].t(), epilogue=Gm.EPI_BIAS_ACT,
                                                                bias=wt[f"b{i}.bfc"], got_f=tr["pl_f"])["C2"], BF16)})
        add("pooled c_proj", lambda wt, tr: {"rows": Out(*_mm(tr["pl_g"], wt[f"b{i}.wproj16"].t(), epilogue=Gm.EPI_RESID_F32,
                                                              bias=wt[f"b{i}.bproj"], resid=tr["pl_x2"])["C"], F32)})
    if sp.pooled:
        pooled_fwd(L - 1)
    else:
        add("gather pooled rows", lambda wt, tr: {"rows": Out(tr[f"x.{L}"][_pool_rows(sp, tr)], None, F32)})

    # ------------------------------------------------------------------------------------------------------------ forward: head
    add("ln_post", lambda wt, tr: {"pooled": Out(*F.norm_fwd(tr["rows"], wt["ln_post_w"], wt["ln_post_b"], EPS)["y_bf16"], BF16)})
    add("proj", lambda wt, tr: {"emb": Out(*_mm(tr["pooled"], wt["proj16"], epilogue=Gm.EPI_F32)["C"], F32)})
    if not backward:
        return S

    # =========================================================================================================== backward: head
    def colsum_depth(rows):
        p = GC.colsum_plan(rows, W, True, sp.scratch)
        return G.colsum_depth(p["rpb"], p["gy"])

    def colsum(x, prior, rows):
        r, b = G.colsum(x, prior, colsum_depth(rows))
        return r.to(x.device), b.to(x.device)

    add("cast demb", lambda wt, tr: {"demb16": Out(tr["demb"], None, BF16)})
    add("proj wgrad", lambda wt, tr: {"g.proj": Out(*_mm(tr["pooled"].double().t(), tr["demb16"], epilogue=Gm.EPI_ATOMIC_F32,
                                                        c0=tr["g0.proj"])["C"], F32)})
    add("proj dgrad", lambda wt, tr: {"dpooled": Out(*_mm(tr["demb16"], wt["proj16"].t(), epilogue=Gm.EPI_BF16)["C"], BF16)})

    def ln_post_bwd(wt, tr):
        nb = F.norm_bwd(tr["rows"], wt["ln_post_w"], tr["dpooled"], EPS, dgamma0=tr["g0.ln_post_w"], dbeta0=tr["g0.ln_post_b"])
        return {"drows": Out(*nb["dx_f32"], F32), "g.ln_post_w": Out(*nb["dgamma"], F32), "g.ln_post_b": Out(*nb["dbeta"], F32)}
    add("ln_post bwd", ln_post_bwd)
    if sp.pooled:
        add("head: bf16 of drows", lambda wt, tr: {"pl_dxb.h": Out(tr["drows"], None, BF16)})
        add(f"head: g_bproj [{L - 1}]", lambda wt, tr: {f"g.b{L - 1}.bproj": Out(*colsum(tr["pl_dxb.h"], tr[f"g0.b{L - 1}.bproj"], M), F32)})
    else:
        def scatter(wt, tr):
            z = torch.zeros(R, W, dtype=tr["drows"].dtype, device=tr["drows"].device)
            return {f"dx.{L}": Out(G.scatter_rows(tr["drows"], _pool_rows(sp, tr), z, 0), None, F32)}
        add("head: scatter", scatter)
        add("head: bf16 of dx", lambda wt, tr: {f"dxb.{L}": Out(tr[f"dx.{L}"], None, BF16)})
        add(f"head: g_bproj [{L - 1}]", lambda wt, tr: {f"g.b{L - 1}.bproj": Out(*colsum(tr[f"dxb.{L}"], tr[f"g0.b{L - 1}.bproj"], R), F32)})

    # ========================================================================================================= backward: blocks
    def wgrad(dy, x, c0, rowsum0=None):
        return _mm(dy.double().t(), x, epilogue=Gm.EPI_ATOMIC_F32, c0=c0, rowsum0=rowsum0)

    def ln2_bwd(x2, gam, df, wfc16, dres, g0w, g0b, g0bo):
        """two stages: d ln_2 out = df @ Wfc (rebuilt), then ln_2's backward"""
        rh, bh = _mm(df, wfc16, epilogue=Gm.EPI_BF16)["C"]
        nb = F.norm_bwd(x2, gam, rh, EPS, dres=dres, dgamma0=g0w, dbeta0=g0b, colsum0=g0bo)
        se = F.norm_bwd_dy_sensitivity(x2, gam, bh, EPS)
        return {k: (nb[k][0], nb[k][1] + se[k]) for k in ("dx_f32", "dgamma", "dbeta", "dx_colsum")}

    def ln1_bwd(i):
        def fn(wt, tr):
            nb = F.norm_bwd(tr[f"x.{i}"], wt[f"b{i}.ln1_w"], tr[f"dh.{i}"], EPS, dres=tr[f"dx2.{i}"], dgamma0=tr[f"g0.b{i}.ln1_w"],
                            dbeta0=tr[f"g0.b{i}.ln1_b"], colsum0=tr[f"g0.b{i - 1}.bproj"] if i > 0 else None)
            out = {f"dx.{i}": Out(*nb["dx_f32"], F32), f"dxb.{i}": Out(*nb["dx_bf16"], BF16),
                   f"g.b{i}.ln1_w": Out(*nb["dgamma"], F32), f"g.b{i}.ln1_b": Out(*nb["dbeta"], F32)}
            if i > 0:
                out[f"g.b{i - 1}.bproj"] = Out(*nb["dx_colsum"], F32)
            return out
        return fn

    def block_bwd(i):
        n, b = i + 1, f"b{i}"

        def c_proj_dgrad(wt, tr):
            r = _mm(tr[f"dxb.{n}"], wt[f"{b}.wproj16"], epilogue=Gm.EPI_DACT, aux=tr[f"f.{i}"], colsum0=tr[f"g0.{b}.bfc"],
                    colsum_rounded=gemm_tile(R, 4 * W, W) == 128)
            return {f"df.{i}": Out(*r["C"], BF16), f"g.{b}.bfc": Out(*r["colsum"], F32)}
        add(f"c_proj dgrad [{i}]", c_proj_dgrad)
        add(f"c_proj wgrad [{i}]", lambda wt, tr: {f"g.{b}.wproj": Out(*wgrad(tr[f"dxb.{n}"], tr[f"g.{i}"], tr[f"g0.{b}.wproj"])["C"], F32)})
        add(f"c_fc wgrad [{i}]", lambda wt, tr: {f"g.{b}.wfc": Out(*wgrad(tr[f"df.{i}"], tr[f"h2.{i}"], tr[f"g0.{b}.wfc"])["C"], F32)})

        def ln2b(wt, tr):
            r = ln2_bwd(tr[f"x2.{i}"], wt[f"{b}.ln2_w"], tr[f"df.{i}"], wt[f"{b}.wfc16"], tr[f"dx.{n}"], tr[f"g0.{b}.ln2_w"],
                        tr[f"g0.{b}.ln2_b"], tr[f"g0.{b}.bo"])
            return {f"dx2.{i}": Out(*r["dx_f32"], F32), f"g.{b}.ln2_w": Out(*r["dgamma"], F32), f"g.{b}.ln2_b": Out(*r["dbeta"], F32),
                    f"g.{b}.bo": Out(*r["dx_colsum"], F32)}
        add(f"c_fc dgrad + ln_2 bwd [{i}]", ln2b)
        add(f"out_proj wgrad [{i}]", lambda wt, tr: {f"g.{b}.wo": Out(*wgrad(r16(tr[f"dx2.{i}"]), tr[f"ao.{i}"], tr[f"g0.{b}.wo"])["C"], F32)})

        def attn_bwd(wt, tr):
            ra, ba = _mm(r16(tr[f"dx2.{i}"]), wt[f"{b}.wo16"], epilogue=Gm.EPI_BF16)["C"]          # d attention out, rebuilt
            qkv, ao, lse = tr[f"qkv.{i}"], tr[f"ao.{i}"], tr[f"lse.{i}"]
            d = qkv.device
            ref, bnd = torch.zeros(R, 3 * W, dtype=torch.float64, device=d), torch.zeros(R, 3 * W, dtype=torch.float64, device=d)
            for m, (s, nn) in enumerate(sp.items()):
                q, k, v = _qkv_item(qkv, s, nn, H)
                valid = A.valid_mask(nn, nn, causal=sp.is_text, device=d)
                oi, li = ao[s:s + nn].reshape(nn, H, 64), lse[m, :, :nn]
                r = A.backward_reference(q, k, v, oi, ra[s:s + nn].reshape(nn, H, 64), li, scale=SCALE, dtype=BF16, valid=valid)
                se = A.backward_dout_sensitivity(q, k, v, oi, li, ba[s:s + nn].reshape(nn, H, 64), scale=SCALE, valid=valid)
                for j, key in enumerate(("dq", "dk", "dv")):
                    ref[s:s + nn, j * W:(j + 1) * W] = r[key][0].reshape(nn, W)
                    bnd[s:s + nn, j * W:(j + 1) * W] = (r[key][1] + se[key]).reshape(nn, W)
            return {f"dqkv.{i}": Out(ref, bnd, BF16)}
        add(f"out_proj dgrad + attention bwd [{i}]", attn_bwd)

        def in_proj_wgrad(wt, tr):
            r = wgrad(tr[f"dqkv.{i}"], tr[f"h1.{i}"], tr[f"g0.{b}.wqkv"], rowsum0=tr[f"g0.{b}.bqkv"])
            return {f"g.{b}.wqkv": Out(*r["C"], F32), f"g.{b}.bqkv": Out(*r["rowsum"], F32)}
        add(f"in_proj wgrad [{i}]", in_proj_wgrad)
        add(f"in_proj dgrad [{i}]", lambda wt, tr: {f"dh.{i}": Out(*_mm(tr[f"dqkv.{i}"], wt[f"{b}.wqkv16"], epilogue=Gm.EPI_BF16)["C"], BF16)})
        add(f"ln_1 bwd [{i}]", ln1_bwd(i))

    def pooled_bwd(i):
        b = f"b{i}"

        def c_proj_dgrad(wt, tr):
            r = _mm(tr["pl_dxb.h"], wt[f"{b}.wproj16"], epilogue=Gm.EPI_DACT, aux=tr["pl_f"], colsum0=tr[f"g0.{b}.bfc"],
                    colsum_rounded=gemm_tile(M, 4 * W, W) == 128)
            return {"pl_df": Out(*r["C"], BF16), f"g.{b}.bfc": Out(*r["colsum"], F32)}
        add("pooled c_proj dgrad", c_proj_dgrad)
        add("pooled c_proj wgrad", lambda wt, tr: {f"g.{b}.wproj": Out(*wgrad(tr["pl_dxb.h"], tr["pl_g"], tr[f"g0.{b}.wproj"])["C"], F32)})
        add("pooled c_fc wgrad", lambda wt, tr: {f"g.{b}.wfc": Out(*wgrad(tr["pl_df"], tr["pl_h2"], tr[f"g0.{b}.wfc"])["C"], F32)})

        def ln2b(wt, tr):
            r = ln2_bwd(tr["pl_x2"], wt[f"{b}.ln2_w"], tr["pl_df"], wt[f"{b}.wfc16"], tr["drows"], tr[f"g0.{b}.ln2_w"],
                        tr[f"g0.{b}.ln2_b"], tr[f"g0.{b}.bo"])
            return {"pl_dx2": Out(*r["dx_f32"], F32), f"g.{b}.ln2_w": Out(*r["dgamma"], F32), f"g.{b}.ln2_b": Out(*r["dbeta"], F32),
                    f"g.{b}.bo": Out(*r["dx_colsum"], F32)}
        add("pooled c_fc dgrad + ln_2 bwd", ln2b)
        add("pooled bf16 of dx2", lambda wt, tr: {"pl_dxb": Out(tr["pl_dx2"], None, BF16)})
        add("pooled out_proj wgrad", lambda wt, tr: {f"g.{b}.wo": Out(*wgrad(tr["pl_dxb"], tr["pl_ao"], tr[f"g0.{b}.wo"])["C"], F32)})
        add("pooled out_proj dgrad", lambda wt, tr: {"pl_dh": Out(*_mm(tr["pl_dxb"], wt[f"{b}.wo16"], epilogue=Gm.EPI_BF16)["C"], BF16)})

        def attn_one_bwd(wt, tr):
            qkv, d = tr[f"qkv.{i}"], tr[f"qkv.{i}"].device
            dq, dqb = torch.zeros(M, W, dtype=torch.float64, device=d), torch.zeros(M, W, dtype=torch.float64, device=d)
            kv, kvb = torch.zeros(R, 2 * W, dtype=torch.float64, device=d), torch.zeros(R, 2 * W, dtype=torch.float64, device=d)
            for m, (s, _) in enumerate(sp.items()):
                kl = _klen(sp, tr, m)
                _, k, v = _qkv_item(qkv, s, kl, H)
                r = A.backward_reference(tr["pl_q"][m].reshape(1, H, 64), k, v, tr["pl_ao"][m].reshape(1, H, 64),
                                         tr["pl_dh"][m].reshape(1, H, 64), tr["pl_lse"][m].reshape(H, 1), scale=SCALE, dtype=BF16,
                                         valid=A.valid_mask(1, kl, device=d))
                dq[m], dqb[m] = r["dq"][0].reshape(W), r["dq"][1].reshape(W)
                for j, key in enumerate(("dk", "dv")):          # (keys behind a caption's EOT: exact zeros, bound 0)
                    kv[s:s + kl, j * W:(j + 1) * W], kvb[s:s + kl, j * W:(j + 1) * W] = r[key][0].reshape(kl, W), r[key][1].reshape(kl, W)
            return {"pl_dqkv": _full(dq, dqb, (M, 3 * W), (slice(None), slice(0, W)), BF16, d),
                    f"dqkv.{i}": _full(kv, kvb, (R, 3 * W), (slice(None), slice(W, 3 * W)), BF16, d)}
        add("pooled attention bwd", attn_one_bwd)

        def kv_wgrad(wt, tr):
            r = wgrad(tr[f"dqkv.{i}"][:, W:], tr[f"h1.{i}"], tr[f"g0.{b}.wqkv"][W:], rowsum0=tr[f"g0.{b}.bqkv"][W:])
            d = tr[f"h1.{i}"].device
            return {f"g.{b}.wqkv": _full(*r["C"], (3 * W, W), slice(W, 3 * W), F32, d),
                    f"g.{b}.bqkv": _full(*r["rowsum"], (3 * W,), slice(W, 3 * W), F32, d)}
        add("pooled K|V in_proj wgrad", kv_wgrad)

        def q_wgrad(wt, tr):
            r = wgrad(tr["pl_dqkv"][:, :W], tr["pl_h1"], tr[f"g0.{b}.wqkv"][:W], rowsum0=tr[f"g0.{b}.bqkv"][:W])
            d = tr["pl_h1"].device
            return {f"g.{b}.wqkv": _full(*r["C"], (3 * W, W), slice(0, W), F32, d),
                    f"g.{b}.bqkv": _full(*r["rowsum"], (3 * W,), slice(0, W), F32, d)}
        add("pooled Q in_proj wgrad", q_wgrad)

        def kv_dgrad(wt, tr):
            r, bd = _mm(tr[f"dqkv.{i}"][:, W:], wt[f"{b}.wqkv16"][W:], epilogue=Gm.EPI_BF16)["C"]
            o = Out(r, bd, BF16, torch.ones(R, W, dtype=torch.bool, device=r.device))
            o.mask[_pool_rows(sp, tr)] = False          # the pooled rows get the K = 3W product below
            return {f"dh.{i}": o}
        add("pooled K|V in_proj dgrad", kv_dgrad)
        add("pooled gather dk|dv", lambda wt, tr: {"pl_dqkv": _full(tr[f"dqkv.{i}"][_pool_rows(sp, tr)][:, W:], None, (M, 3 * W),
                                                                    (slice(None), slice(W, 3 * W)), BF16, tr["pl_dqkv"].device)})
        add("pooled in_proj dgrad, K = 3W", lambda wt, tr: {"pl_dhq": Out(*_mm(tr["pl_dqkv"], wt[f"{b}.wqkv16"], epilogue=Gm.EPI_BF16)["C"], BF16)})
        add("pooled rows of dh", lambda wt, tr: {f"dh.{i}": _full(tr["pl_dhq"], None, (R, W), _pool_rows(sp, tr), BF16, tr["pl_dhq"].device)})

        def scatter(wt, tr):
            z = torch.zeros(R, W, dtype=tr["pl_dx2"].dtype, device=tr["pl_dx2"].device)
            return {f"dx2.{i}": Out(G.scatter_rows(tr["pl_dx2"], _pool_rows(sp, tr), z, 0), None, F32)}
        add("pooled scatter dx2", scatter)
        add(f"ln_1 bwd [{i}]", ln1_bwd(i))

    for i in range(L - 1, -1, -1):
        (pooled_bwd if sp.pooled and i == L - 1 else block_bwd)(i)

    # =========================================================================================================== backward: stem
    if sp.is_text:
        def tok_bwd(wt, tr):
            lens = torch.tensor(sp.lens) if sp.lens else None
            plan = GC.tokd_plan(R, sp.vocab, W, True, True, sp.scratch)
            r, bd = G.dtok(tr["input"], tr["dx.0"], sp.vocab, tr["g0.tok"], plan["form"] != "atomic", lens, plan["nslices"])
            d = tr["dx.0"].device
            pos = G.text_dpos(tr["dx.0"], M, T, tr["g0.pos"], None if lens is None else lens.to(d))
            return {"g.tok": Out(r.to(d), bd.to(d), F32), "g.pos": Out(pos, None, F32)}
        add("text_embed bwd", tok_bwd)
        return S

    def ln_pre_bwd(wt, tr):
        nb = F.norm_bwd(tr["x0"], wt["ln_pre_w"], tr["dx.0"], EPS, dgamma0=tr["g0.ln_pre_w"], dbeta0=tr["g0.ln_pre_b"])
        return {"dx0": Out(*nb["dx_f32"], F32), "g.ln_pre_w": Out(*nb["dgamma"], F32), "g.ln_pre_b": Out(*nb["dbeta"], F32)}
    add("ln_pre bwd", ln_pre_bwd)

    def assemble_bwd(wt, tr):
        r = G.vit_assemble_bwd(tr["dx0"], M, T, tr["g0.cls"], tr["g0.pos"])
        return {"dpo": Out(r["dpatch"], None, BF16), "g.cls": Out(r["dclass"], None, F32), "g.pos": Out(r["dpos"], None, F32)}
    add("vit_assemble bwd", assemble_bwd)
    add("conv wgrad", lambda wt, tr: {"dconv": Out(*wgrad(tr["dpo"], tr["patches"], torch.zeros(W, sp.kpad, device=tr["dpo"].device))["C"], F32)})
    add("unpad_add", lambda wt, tr: {"g.conv": Out(tr["g0.conv"] + tr["dconv"][:, :3 * sp.patch * sp.patch], None, F32)})
    return S


# ================================================================================================================ compose / verify
def _stored(o, exact):
    if o.dt == I32:
        return o.ref.to(I32)
    return o.ref.double() if exact else o.ref.to(o.dt)


def compose(sp, wt, tr, backward=True, exact=False):
    """chain the stage references end to end: every stage reads what the stages before it stored.  tr holds input (and demb and the
    g0.* priors for the backward) and is filled in place.  exact: float64 throughout, nothing is rounded (the weights under <name>16
    are then the unrounded masters) -- the operation itself, which tests/test_tower_ref.py compares with the oracle's autograd"""
    for _, fn in stages(sp, backward):
        for name, o in fn(wt, tr).items():
            new = _stored(o, exact)
            if o.mask is not None and name in tr:
                new = torch.where(o.mask, new, tr[name])
            elif o.mask is not None:
                new = torch.where(o.mask, new, torch.zeros_like(new))
            tr[name] = new
    return tr


def judge(got, o):
    """-> (ratio, verdict): the comparer of every tower stage test.  ratio = worst |got - ref| / bound over the stage's elements (inf:
    outside the bound, NaN / Inf, or -- for a bit-exact stage -- any differing bit); verdict None when accepted, else the reason"""
    dev = o.ref.device
    got = got.to(dev)
    if tuple(got.shape) != tuple(o.ref.shape):
        return math.inf, f"shape {tuple(got.shape)} instead of {tuple(o.ref.shape)}"
    if o.bound is None:
        want = o.ref.to(got.dtype)
        a, b = G.ibits(got), G.ibits(want)
        if o.mask is not None:
            a, b = a[o.mask], b[o.mask]
        bad = int((a != b).sum())
        return (math.inf, f"{bad} of {a.numel()} elements differ in their bits") if bad else (0.0, None)
    g, r, b = got.double(), o.ref, o.bound
    if o.mask is not None:
        g, r, b = g[o.mask], r[o.mask], b[o.mask]
    ratio = A.worst(g, r, b)
    if not ratio <= 1.0:
        bad = Gm.violations(g, r, b)
        d = (g - r).abs()
        fin = d[torch.isfinite(d)]
        return math.inf, (f"{int(bad.sum())} of {bad.numel()} elements outside the bound (largest finite |got - ref| "
                          f"{float(fin.max()) if fin.numel() else math.nan:.3g}, median bound {float(b.median()):.3g})")
    return ratio, None


def verify(sp, wt, tr, backward=True, only=None, bounds=None):
    """judge every stage output held by the trace against its stage reference evaluated on the TRACE's own inputs.
    -> [(stage label, trace name, ratio, verdict)]; outputs the trace does not hold are skipped and listed with verdict "absent".
    bounds (a dict): filled with name -> the bound of every bounded output (parts of one tensor added up)"""
    res = []
    for label, fn in stages(sp, backward):
        if only is not None and not only(label):
            continue
        for name, o in fn(wt, tr).items():
            if name not in tr:
                res.append((label, name, 0.0, "absent"))
                continue
            res.append((label, name) + judge(tr[name], o))
            if bounds is not None and o.bound is not None:
                bounds[name] = o.bound if name not in bounds else bounds[name] + o.bound
    return res


def failures(res):
    return [r for r in res if r[3] is not None]


# ======================================================================================================================= mutations
def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _m_bqkv_k_garbage(sp, wt, tr):
    i, W = sp.L - 1, sp.W
    g = tr[f"g.b{i}.bqkv"]
    g[W:2 * W] += 1e-3 * torch.randn(W, generator=_gen(1)).to(g)


def _m_pos_row(sp, wt, tr):
    g = tr["g.pos"]
    g[3] = tr["g0.pos"][3] + (g[4] - tr["g0.pos"][4])


def _m_q_bias_missing(sp, wt, tr):
    i, W = sp.L - 1, sp.W
    tr[f"g.b{i}.bqkv"][:W] = tr[f"g0.b{i}.bqkv"][:W]


def _m_q_bias_twice(sp, wt, tr):
    i, W = sp.L - 1, sp.W
    g, g0 = tr[f"g.b{i}.bqkv"], tr[f"g0.b{i}.bqkv"]
    g[:W] = g0[:W] + 2 * (g[:W] - g0[:W])


def _m_dh_from_kv_only(sp, wt, tr):
    i, W = sp.L - 1, sp.W
    rows = _pool_rows(sp, tr)
    kv = tr[f"dqkv.{i}"][rows][:, W:].double() @ wt[f"b{i}.wqkv16"][W:].double()
    tr[f"dh.{i}"][rows] = kv.to(tr[f"dh.{i}"].dtype)


def _m_bproj_wrong_ln(sp, wt, tr):
    i = 1          # (with a pooled block 1 its dx2 is the scattered pl_dx2: just as wrong a source)
    tr[f"g.b{i - 1}.bproj"] = (tr[f"g0.b{i - 1}.bproj"].double() + r16(tr[f"dx2.{i}"]).double().sum(0)).to(tr[f"g.b{i - 1}.bproj"].dtype)


def _m_resid_rows(sp, wt, tr):
    x2, x = tr["x2.0"], tr["x.0"]
    for r in (3, 4, 5):
        x2[r] = (x2[r].double() - x[r].double() + x[r + 1].double()).to(x2.dtype)


def _m_kv_bias_shifted(sp, wt, tr):
    i, W = sp.L - 1, sp.W
    b = wt[f"b{i}.bqkv"].double()
    q = tr[f"qkv.{i}"]
    q[:, W:] = (q[:, W:].double() - b[W:] + torch.roll(b[W:], 64)).to(q.dtype)


def _m_wqkv_grad_shifted(sp, wt, tr):
    # the K | V weight gradient written one 64-row block too early: g_wqkv + W*W - 64*W
    i, W = sp.L - 1, sp.W
    g, g0 = tr[f"g.b{i}.wqkv"], tr[f"g0.b{i}.wqkv"]
    d = (g - g0)[W:].clone()
    g[W:] = g0[W:]
    g[W - 64:3 * W - 64] = g[W - 64:3 * W - 64] + d


def _m_pool_index(sp, wt, tr):
    rows = _pool_rows(sp, tr)
    if sp.pooled:
        tr["pl_h1"] = tr[f"h1.{sp.L - 1}"][rows - 1].clone()
    else:
        tr["rows"] = tr[f"x.{sp.L}"][rows - 1].clone()


def _m_bias_twice(sp, wt, tr):
    x2 = tr["x2.0"]
    tr["x2.0"] = (x2.double() + wt["b0.bo"].double()).to(x2.dtype)


# (name, needs a pooled last block: True / False / None = either, the defect).  tests/test_tower_ref.py lists the cases of each
MUTATIONS = [
    ("garbage in the K third of g_bqkv", None, _m_bqkv_k_garbage),
    ("one wrong row of g_pos", None, _m_pos_row),
    ("pooled block: Q-part bias gradient missing", True, _m_q_bias_missing),
    ("pooled block: Q-part bias gradient counted twice", True, _m_q_bias_twice),
    ("pooled rows' dh from the K|V-only product", True, _m_dh_from_kv_only),
    ("g_bproj of the block before summed from ln_2's dxb", None, _m_bproj_wrong_ln),
    ("wrong residual operand on three rows", None, _m_resid_rows),
    ("pooled block: K|V bias one column block off", True, _m_kv_bias_shifted),
    ("pooled block: K|V weight gradient one row block off", True, _m_wqkv_grad_shifted),
    ("pooled index off by one", None, _m_pool_index),
    ("out_proj bias added twice", None, _m_bias_twice),
]
