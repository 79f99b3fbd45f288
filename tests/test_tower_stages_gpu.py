"""The CLIP tower calls (csrc/tower.hip) judged stage by stage: every launch of uniir_clip_tower_fwd, _bwd_head, _bwd_blocks (one
block per call) and _bwd_stem against its stage reference of tests/tower_ref.py, evaluated on the DEVICE's own inputs to that launch
and gated by the element-wise bounds of the per-kernel references (gemm_ref, attention_ref, fp32_ref, glue_ref) -- nothing wider.

The test calls the C ABI with its own buffers.  Weights, every gradient target, the embeddings, demb, the input and the workspace
sit in NaN-patterned, guard-banded buffers (fp32_cases.Buf); every gradient buffer starts from non-zero contents (the contract is
+=).  The intermediates are read out of the workspace through uniir_clip_tower_layout, the backward transients between the calls.
Checked besides the stages: weights and inputs come back bit for bit; nothing outside a logical extent changes (the gaps between the
workspace's regions, the guard behind `total`, the guard rows of every buffer, the Q columns of the pooled block's qkv); the forward
stash survives the backward bit for bit; the one-call backward on a fresh workspace gives the staged run's gradients bit for bit
where no float atomics are involved (a second run gives the same bits again) and within the summed bound elsewhere; a packed text
case gives its dense twin's embeddings and activation gradients bit for bit on the live rows.

stash_act is 1 throughout (act(f) of every layer is then a readable stage output); ln_bwd_side is the default of
uniir_amd.clip_model (1) and, for V1 and V2, once 0.  Recompute, the forward-only ping-pong and fp16 are tied to this mode by the
existing mode-against-mode tests.

Each case prints one OBS line per stage family with the worst |got - ref| / bound (profiles/tower_stages.txt holds a run's lines).
Worst ratios observed on an MI355X over all cases, per stage family (full block / pooled last block):
  bit-exact stages (patchify, vit_assemble{,_bwd}, text_embed, text g_pos, gathers, scatters, casts, unpad_add)      0 differing bits
  GEMMs with a bf16 output: conv 0.86, in_proj 0.99 / 0.98, c_fc 0.99 / 0.96, act(f) 0.99 / 0.99, proj dgrad 0.98,
      c_proj dgrad 0.98 / 0.95, out_proj dgrad - / 0.95, in_proj dgrad 0.96 / 0.97 (K = 3W on the pooled rows 0.90)
  GEMMs with an fp32 output: out_proj 0.014 / 0.007, c_proj 0.003 / 0.002, proj 0.004
  weight gradients (fp32, +=): proj 0.11, c_proj 0.03 / 0.12, c_fc 0.03 / 0.15, out_proj 0.03 / 0.16, in_proj 0.02 / K|V 0.02, Q 0.12,
      conv 0.02; bias sums: g_bproj from the head 0.02, token gradient 0.34
  LayerNorm forward (bf16 out): ln_1 0.50, ln_2 0.50 / 0.50, ln_post 0.49; ln_pre (fp32 out) 0.05
  LayerNorm backward: ln_post 0.09, ln_pre 0.07, ln_1 (with dxb, g_ln1, the previous block's g_bproj) 0.50
  attention forward 0.40 / one query 0.33; attention backward behind the rebuilt out_proj dgrad 0.52 / one query (single stage) 0.49
  ln_2 backward behind the rebuilt c_fc dgrad (dx2, g_ln2, g_bo) 0.75 / 0.75
Why some sit near 1 and that is right: gemm_ref bounds a 16-bit store by u |v| with u = 2^-8, which is exactly what a correctly
rounded bf16 store attains when the value lies just above a power of two -- that reference has no safety factor on the output
rounding (the norms carry MARGIN = 2 and attention C = 2, hence their 0.5), and tests/test_gemm_paths_gpu.py sees the same figures.
Over a few hundred thousand elements some element always comes close.  The ln_2 two-stage check inherits it: the rebuilt d ln_2 out
differs from the device's by that tensor's own bf16 rounding, and the dominant term of dx2 is rstd gamma times it.  The fp32 outputs,
whose bounds hold only accumulation error, sit at a few per cent or less.
"""
import ctypes as C
import re

import pytest
import torch

import fp32_cases as FC
import tower_cases as TC
import tower_ref as TR
from tower_cases import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32, I32 = torch.bfloat16, torch.float32, torch.int32
WS_GUARD = 1 << 16
PATTERN = 0x7FC1          # every 16 bits of the workspace before the forward: a bf16 NaN, an fp32 NaN as a pair

# trace name -> (layout field, dtype, shape); i: the layer whose set holds it
LAYER = {"x": ("o_x", F32, "RW"), "h1": ("o_h1", BF16, "RW"), "qkv": ("o_qkv", BF16, "R3W"), "ao": ("o_ao", BF16, "RW"),
         "lse": ("o_lse", F32, "MHT"), "x2": ("o_x2", F32, "RW"), "h2": ("o_h2", BF16, "RW"), "f": ("o_f", BF16, "R4W"),
         "g": ("o_g", BF16, "R4W")}
FWD_FLAT = {"patches": ("patches", BF16, "PK"), "po": ("po", BF16, "PW"), "x0": ("x0", F32, "RW"), "eot": ("eot", I32, "M"),
            "rows": ("pooled_rows", F32, "MW"), "pooled": ("pooled", BF16, "MW"), "pl_h1": ("pl_h1", BF16, "MW"), "pl_q": ("pl_q", BF16, "MW"),
            "pl_ao": ("pl_ao", BF16, "MW"), "pl_lse": ("pl_lse", F32, "MH"), "pl_x": ("pl_x", F32, "MW"), "pl_x2": ("pl_x2", F32, "MW"),
            "pl_h2": ("pl_h2", BF16, "MW"), "pl_f": ("pl_f", BF16, "M4W"), "pl_g": ("pl_g", BF16, "M4W")}
HEAD = {"demb16": ("demb16", BF16, "ME"), "dpooled": ("dpooled", BF16, "MW"), "drows": ("drows", F32, "MW")}
BLOCK = {"df": ("df", BF16, "R4W"), "dh": ("dh", BF16, "RW"), "dx2": ("dx2", F32, "RW"), "dqkv": ("dqkv", BF16, "R3W"),
         "dx": ("dx", F32, "RW"), "dxb": ("dxb", BF16, "RW")}
POOLED_BWD = {"pl_df": ("pl_df", BF16, "M4W"), "pl_dx2": ("pl_dx2", F32, "MW"), "pl_dxb": ("pl_dxb", BF16, "MW"),
              "pl_dh": ("pl_dh", BF16, "MW"), "pl_dqkv": ("pl_dqkv", BF16, "M3W"), "pl_dhq": ("pl_dhq", BF16, "MW")}
STEM = {"dx0": ("dx0", F32, "RW"), "dpo": ("dpo", BF16, "PW"), "dconv": ("dconv", F32, "WK")}


def _shape(sp, code):
    R, W, M = sp.R, sp.W, sp.M
    return {"RW": (R, W), "R3W": (R, 3 * W), "R4W": (R, 4 * W), "MHT": (M, sp.H, sp.T), "PK": (M * sp.G, sp.kpad), "PW": (M * sp.G, W),
            "M": (M,), "MW": (M, W), "MH": (M, sp.H), "M4W": (M, 4 * W), "M3W": (M, 3 * W), "ME": (M, sp.E), "WK": (W, sp.kpad)}[code]


def _buf(t):
    """a tensor in a NaN-patterned, guard-banded buffer of its own dtype"""
    t2 = t.reshape(1, -1) if t.dim() == 1 else t.reshape(t.shape[0], -1)
    return FC.Buf(t2.shape[0], t2.shape[1], dtype=t.dtype, device=DEV).set(t2)


_STREAM = []


def _stream_handle():
    """one stream of its own for every call of this file, with the reduction scratch that uniir_amd.ops attaches to the streams it
    launches on (fixed-order bias / LayerNorm / token-gradient sums).  Registered through ops and left registered: ops keeps the
    table of which stream has which buffer, and a registration behind its back would leave later tests on atomics"""
    from uniir_amd import ops
    if not _STREAM:
        _STREAM.append(torch.cuda.Stream())
    with torch.cuda.stream(_STREAM[0]):
        return ops._stream()


class Run:
    """one tower description with its buffers; fwd() and the staged or one-call backward fill self.tr"""

    def __init__(self, sp, ln_bwd_side=TC.LN_BWD_SIDE_DEFAULT, splitk="slab", seed=0):
        from uniir_amd import _lib
        self.sp, self.lib, self._lib = sp, _lib.load(), _lib
        self.wt = TC.make_weights(sp, seed, DEV)
        self.tr = TC.trace_inputs(sp, seed, DEV)
        self.bufs = {}
        for k, v in self.wt.items():
            self.bufs[k] = _buf(v)
        for name in sp.params():
            self.bufs["g." + name] = _buf(self.tr["g0." + name])
        inp = self.tr["input"]
        self.bufs["input"] = _buf(inp.reshape(sp.M, -1))
        self.bufs["demb"] = _buf(self.tr["demb"])
        self.bufs["emb"] = FC.Buf(sp.M, sp.E, device=DEV)
        W = sp.W
        need = 4 * 2 * 4 * W * W          # the largest product of the case at the 2 slabs its rows get (V2, T2); others ask for less
        self.splitk_bytes = {"slab": 64 << 20, "none": 0, "short": need - 1}[splitk]
        self.splitk = torch.full(((64 << 20) + WS_GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
        self.row_off = None
        if sp.lens:
            self.row_off = torch.tensor([0] + [s + n for s, n in sp.items()], dtype=I32, device=DEV)
        self.t, self.keep = TC.describe(sp, lambda n: self.bufs[n].view.data_ptr(), ln_bwd_side=ln_bwd_side, stash_act=1,
                                        splitk=(self.splitk.data_ptr() if self.splitk_bytes else None, self.splitk_bytes))
        self.lay = _lib.clip_tower_layout(self.t, sp.M, sp.R if sp.lens else -1, 1)
        self.ws = torch.empty((self.lay.total + WS_GUARD) // 2, dtype=torch.int16, device=DEV).fill_(PATTERN)
        assert self.ws.data_ptr() % 256 == 0
        self.before = {k: b.bits().clone() for k, b in self.bufs.items()}
        torch.cuda.synchronize()

    # ------------------------------------------------------------------------------------------------------------------ calls
    def call(self, fn, *args):
        lib, t, sp = self.lib, C.byref(self.t), self.sp
        packed = (self.row_off.data_ptr(), sp.R) if sp.lens else ()
        handle = _stream_handle()
        wsargs = (self.ws.data_ptr(), self.lay.total, handle)
        inp, demb, emb = (self.bufs[k].view.data_ptr() for k in ("input", "demb", "emb"))
        sfx = "_packed" if sp.lens else ""
        if fn == "fwd":
            rc = getattr(lib, "uniir_clip_tower_fwd" + sfx)(t, inp, sp.M, *packed, emb, self.ws.data_ptr(), self.lay.total, 1, handle)
        elif fn == "head":
            rc = getattr(lib, "uniir_clip_tower_bwd_head" + sfx)(t, demb, sp.M, *packed, *wsargs)
        elif fn == "blocks":
            rc = getattr(lib, "uniir_clip_tower_bwd_blocks" + sfx)(t, sp.M, *packed, args[0], args[1], *wsargs)
        elif fn == "stem":
            rc = getattr(lib, "uniir_clip_tower_bwd_stem" + sfx)(t, inp, sp.M, *packed, *wsargs)
        else:
            assert fn == "bwd" and not sp.lens
            rc = lib.uniir_clip_tower_bwd(t, inp, demb, sp.M, *wsargs)
        self._lib.check(rc, fn)
        torch.cuda.synchronize()

    def read(self, field, dtype, code, layer=None):
        off = getattr(self.lay, field)
        assert off >= 0, field
        if layer is not None:
            off += self.lay.lay0 + layer * self.lay.lay_stride
        shape = _shape(self.sp, code)
        n = 1
        for s in shape:
            n *= s
        assert off % 2 == 0 and off + n * dtype.itemsize <= self.lay.total
        return self.ws[off // 2: off // 2 + n * dtype.itemsize // 2].view(dtype).view(shape).clone()

    def snap(self, table, suffix=""):
        for name, (field, dtype, code) in table.items():
            if getattr(self.lay, field) >= 0:
                self.tr[name + suffix] = self.read(field, dtype, code)
                self.src[name + suffix] = (field, dtype, code)

    def snap_layers(self):
        sp = self.sp
        for i in range(sp.L):
            last_pooled = sp.pooled and i == sp.L - 1
            for name, (field, dtype, code) in LAYER.items():
                if last_pooled and name not in ("x", "h1", "qkv"):
                    continue
                self.tr[f"{name}.{i}"] = self.read(field, dtype, code, i)
                self.src[f"{name}.{i}"] = (field, dtype, code, i)
        if not sp.pooled:
            self.snap({f"x.{sp.L}": ("x_last", F32, "RW")})

    def forward(self):
        self.src = {}
        self.call("fwd")
        self.snap(FWD_FLAT)
        if not self.sp.is_text:
            self.tr.pop("eot")          # a vision tower writes none
        self.snap_layers()
        self.tr["emb"] = self.bufs["emb"].view.clone()
        self.fwd_stash = {k: (src, self.tr[k]) for k, src in self.src.items() if k in self.tr}

    def grads(self):
        for name in self.sp.params():
            self.tr["g." + name] = self.bufs["g." + name].view.reshape(self.tr["g0." + name].shape).clone()

    def backward_staged(self):
        sp, L = self.sp, self.sp.L
        self.call("head")
        self.snap(HEAD)
        if sp.pooled:
            self.tr["pl_dxb.h"] = self.read("pl_dxb", BF16, "MW")
        else:
            self.tr[f"dx.{L}"], self.tr[f"dxb.{L}"] = self.read("dx", F32, "RW"), self.read("dxb", BF16, "RW")
        for i in range(L - 1, -1, -1):
            self.call("blocks", i, i + 1)
            if sp.pooled and i == L - 1:
                self.snap(POOLED_BWD)
                self.snap({k: v for k, v in BLOCK.items() if k != "df"}, f".{i}")
            else:
                self.snap(BLOCK, f".{i}")
        self.call("stem")
        if not sp.is_text:
            self.snap(STEM)
        self.grads()

    def backward_one_call(self):
        if self.sp.lens:          # (no packed one-call entry point: the three stages in one go)
            self.call("head")
            self.call("blocks", 0, self.sp.L)
            self.call("stem")
        else:
            self.call("bwd")
        self.grads()

    # ------------------------------------------------------------------------------------------------------- memory discipline
    def check_untouched(self):
        sp = self.sp
        for k, b in self.bufs.items():
            if k.startswith("g.") or k == "emb":
                b.assert_outside_untouched(self.before[k], k)
            else:
                assert torch.equal(b.bits(), self.before[k]), f"{k}: an input of the tower was written"
        held = torch.zeros(self.ws.numel(), dtype=torch.bool, device=DEV)
        for name, off, nbytes in TC.regions(sp, self.lay):
            held[off // 2:(off + nbytes + 1) // 2] = True
        assert bool((self.ws[~held] == PATTERN).all()), "written outside every region of the layout, or behind `total`"
        assert bool((self.splitk[self.splitk_bytes:] == 0x5A).all()), "written behind the split-K workspace"
        if sp.pooled:          # the pooled block's Q projection lives in pl_q: the Q columns of its qkv stay as they were
            q = self.read("o_qkv", BF16, "R3W", sp.L - 1)[:, :sp.W]
            assert bool((q.view(torch.int16) == PATTERN).all()), "Q columns of the pooled block's qkv were written"
        for k, (src, v) in self.fwd_stash.items():
            assert torch.equal(TR.G.ibits(self.read(*src)), TR.G.ibits(v)), f"{k}: the forward's stash changed during the backward"


def _family(label):
    return re.sub(r" \[\d+\]", "", label)


def _report(case, res):
    fam = {}
    for label, name, ratio, verdict in res:
        f = _family(label)
        fam[f] = max(fam.get(f, 0.0), ratio)
    for f, r in fam.items():
        print(f"OBS case={case} stage={f!r} worst_ratio={r:.3f}")
    return fam


_DONE = {}


def _staged(case, ln_bwd_side=TC.LN_BWD_SIDE_DEFAULT, splitk="slab"):
    key = (case, ln_bwd_side, splitk)
    if key not in _DONE:
        run = Run(CASES[case], ln_bwd_side, splitk)
        run.forward()
        run.backward_staged()
        _DONE.clear()          # one run's tensors at a time, plus the twin a packed case asks for right after
        _DONE[key] = run
    return _DONE[key]


def _check_case(case, ln_bwd_side=TC.LN_BWD_SIDE_DEFAULT, splitk="slab", one_call=True):
    sp = CASES[case]
    tag = case + ("" if ln_bwd_side == TC.LN_BWD_SIDE_DEFAULT else f"-side{ln_bwd_side}") + ("" if splitk == "slab" else f"-splitk-{splitk}")
    run = _staged(case, ln_bwd_side, splitk)
    bounds = {}
    res = TR.verify(sp, run.wt, run.tr, bounds=bounds)
    _report(tag, res)
    bad = TR.failures(res)
    assert not bad, f"{tag}: " + "; ".join(f"{b[0]} -> {b[1]}: {b[3]}" for b in bad[:8])
    run.check_untouched()
    if not one_call:
        return
    # the one-call backward on a fresh workspace and fresh gradient buffers, twice.  Sums without float atomics: the same bits in all
    # three runs.  ATOMIC names the gradients whose split-K slabs are added by atomics for want of slab room: within the summed bound
    atomic = ATOMIC[splitk]
    other = []
    for _ in range(2):
        r2 = Run(sp, ln_bwd_side, splitk)
        r2.forward()
        r2.backward_one_call()
        other.append(r2)
    assert torch.equal(other[0].tr["emb"], run.tr["emb"])
    for name in sp.params():
        a, b = run.tr["g." + name], other[0].tr["g." + name]
        if name.split(".")[-1] not in atomic:
            assert torch.equal(a, b), f"{tag}: g.{name} of the staged and the one-call backward differ"
            assert torch.equal(b, other[1].tr["g." + name]), f"{tag}: g.{name} differs between two runs"
        elif name == "conv":          # one exact fp32 addition onto dconv
            tol = 2 * bounds["dconv"][:, :a.shape[1]] + 2.0 ** -23 * a.double().abs()
            assert bool(((a.double() - b.double()).abs() <= tol).all()), f"{tag}: g.conv staged vs one call"
        else:
            assert bool(((a.double() - b.double()).abs() <= 2 * bounds["g." + name]).all()), f"{tag}: g.{name} staged vs one call"


# the weight gradients that fall back to float atomics: none with slab room for every product; without a workspace every product the
# rows split (and the in_proj bias, summed by the same launches); one byte short of the largest product's slabs, the two 4W x W ones
ATOMIC = {"slab": (), "short": ("wfc", "wproj"), "none": ("wqkv", "bqkv", "wo", "wfc", "wproj", "conv")}

CASE_PARAMS = [(c, TC.LN_BWD_SIDE_DEFAULT, "slab") for c in sorted(CASES)]
CASE_PARAMS += [("V1-pool0", 0, "slab"), ("V2-pool0", 0, "slab"), ("V2-pool1", 0, "slab")]
CASE_PARAMS += [("V2-pool0", TC.LN_BWD_SIDE_DEFAULT, "none"), ("V2-pool0", TC.LN_BWD_SIDE_DEFAULT, "short"), ("V2-pool1", TC.LN_BWD_SIDE_DEFAULT, "none")]


@pytest.mark.parametrize("case,ln_bwd_side,splitk", CASE_PARAMS, ids=[f"{c}-side{s}-{k}" for c, s, k in CASE_PARAMS])
def test_tower_stages(case, ln_bwd_side, splitk):
    _check_case(case, ln_bwd_side, splitk)


@pytest.mark.parametrize("case", [c for c in sorted(CASES) if "packed" in c])
def test_packed_rows_are_the_dense_rows_bit_for_bit(case):
    """the header's promise for the packed text tower: embeddings and activation gradients are bitwise those of the dense call on
    the live rows (weight gradients are the same sums over fewer terms: judged by their own stages above)"""
    sp = CASES[case]
    packed = _staged(case).tr
    packed = {k: v for k, v in packed.items()}
    dense_case = case.replace("packed", "dense")
    dense = _staged(dense_case).tr
    live = TR.G.live_mask(torch.tensor(sp.lens, device=DEV), sp.T).flatten()
    assert torch.equal(packed["emb"], dense["emb"]), "embeddings"
    names = [f"{n}.{i}" for i in range(sp.L) for n in ("dx", "dxb", "dqkv", "dx2", "dh")]
    for name in names:
        a, b = packed[name], dense[name][live]
        if sp.pooled and name == f"dqkv.{sp.L - 1}":
            a, b = a[:, sp.W:], b[:, sp.W:]
        assert torch.equal(TR.G.ibits(a), TR.G.ibits(b)), f"{name}: packed differs from the dense call on live rows"
