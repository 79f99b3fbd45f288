"""The attention entry points of the C ABI on every dispatch path against the fp64 reference of tests/attention_ref.py, element by
element.  Each case names the kernel instantiations it is meant to reach; the path conditions, from launch_attn_fwd /
launch_attn_bwd (csrc/attention.hip), ap_geom (attention_pair.hip) and launch_attn_long_* (attention_long.hip):
  forward   attn_fwd_kernel<REL, DROP, F16>: REL = a relative bias (uniir_attention_rel_*), DROP = drop_p > 0, F16 =
            uniir_attention_fwd_f16; tq, tk <= 512.  32-key blocks, 16-row query tiles dealt over 8 waves; stage_two issues
            ceil(Tkp * 8 / 512) loads per thread in the instantiations <= 2 (Tkp <= 128), <= 5 (Tkp <= 320), 8 (above), Tkp = tk rounded
            up to 32.  Packed rows (row_off) and key_len are run-time arguments of the same kernels.
            attn_long_fwd_kernel<F16>: uniir_attention_fwd / _fwd_f16, plain, 513 .. 1024 tokens, 128 queries per workgroup, K / V
            streamed in 128-key chunks.
  backward  attn_bwd_pair_kernel<224 | 288>: plain self-attention (no mask, key_len, packed rows, bias or dropout), every ld a
            multiple of 8, and ap_geom: an odd number of 16-row tiles, 32 * (tiles / 2) <= T, T % 32 != 0, the odd tile's partial sums
            inside the 160 KiB of LDS: nvl = T - 192 <= 7 at the 224 padding, nvl = 1 at 288 -- exactly T in {193 .. 199, 257}
            (checked here by _pair_takes, a restatement of ap_geom).  One persistent workgroup per compute unit walks the (item, head)
            pairs.
            attn_bwd_kernel<REL, DROP, CAUSAL, NT>: everything else up to 512 tokens; NT = 384 when max(tq, tk) <= 128, else 512 (and
            then the legacy one-slice staging); CAUSAL excludes REL.
            attn_long_dkdv_kernel + attn_long_dq_kernel: uniir_attention_bwd, plain, 513 .. 1024 tokens (64-query / 128-key chunks).
Calls go through the ctypes handle with the test's own buffers: every tensor has a guard band behind it, every leading dimension
the entry point leaves to the caller is wider than the row, and everything outside the logical extent -- the lse entries of the dead
rows of packed items included -- holds a NaN pattern that must come back bit for bit; NaN next to an input must not reach a result.
The operands come from attention_ref.build_items: rows that stress the mask edge, masked positions that would dominate, an early
and a late spike.  The backward runs on the rounded REFERENCE out / lse, so it is judged on its own; cases marked `chained` run it
once more on the kernel's own forward results.  Everything except drel (float atomics) is run twice and compared with torch.equal.
Packed cases are also compared bit for bit, live rows only, with the dense padded call.  Each case prints an OBS line with the largest
|got - ref| / bound of every output (profiles/attention_paths.txt keeps a run's lines).
The contract excludes key_len[m] < 1 and packed items without rows (include/uniir_hip.h); no case passes either."""
import ctypes as C
import faulthandler

import pytest
import torch

import attention_ref as R
from attention_ref import Case

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 24            # rows of guard band behind every tensor
TAIL = 64             # spare floats behind lse / drel
PAD = 72              # extra elements of a leading dimension the caller chooses (multiple of 8)
NAN16 = {torch.bfloat16: 0x7FC1, torch.float16: 0x7E01}
NAN32 = 0x7FC00011
ERR = {"EINVAL": -1, "ESHAPE": -2, "EALIGN": -3}
DROP_SEED = 4242
CASE_SECONDS = 120    # a case takes a few seconds; a hung kernel ends the run here instead of at the runner's limit

BF, F16 = torch.bfloat16, torch.float16


# ----------------------------------------------------------------------------------------------------------------- the case table
def _pair_takes(T):
    """ap_geom of csrc/attention_pair.hip"""
    if T <= 192 or T > 288:
        return False
    tp = 224 if T <= 224 else 256 if T <= 256 else 288
    nt = (T + 15) // 16
    npair, left = nt // 2, nt % 2
    nvl = T - 32 * npair if left else 1
    return tp != 256 and npair <= 8 and 32 * npair <= T and T % 32 != 0 and 4 * tp * 128 + 4 * tp * 4 + 8 * 3 * nvl * 64 * 4 <= 160 * 1024


assert [T for T in range(1, 513) if _pair_takes(T)] == [193, 194, 195, 196, 197, 198, 199, 257]


def _nt(tmax):
    return 384 if tmax <= 128 else 512


def _nl(tk):
    n = -(-((tk + 31) // 32 * 32 * 8) // 512)
    return 2 if n <= 2 else 5 if n <= 5 else 8


CASES = []
# general forward (bf16 with its backward, fp16 forward only), plain and causal, at every size where a block, a tile, a staging
# instantiation or the backward's thread count changes
for T in (1, 15, 16, 17, 31, 32, 33, 64, 65, 128, 129, 145, 320, 321, 512):
    for causal in (False, True):
        cz = "causal" if causal else "plain"
        CASES.append(Case(f"self-{cz}-{T}", f"attn_fwd_kernel<0,0,0> NL{_nl(T)} + attn_bwd_kernel<0,0,{int(causal)},{_nt(T)}>", "qkv",
                          2, 2 + (T % 2), T, causal=causal, chained=T in (17, 145)))
        CASES.append(Case(f"f16-{cz}-{T}", f"attn_fwd_kernel<0,0,1> NL{_nl(T)}", "f16", 2, 2 + (T % 2), T, causal=causal))
# key_len at every block / tile edge, with and without the causal mask, under and over 128 tokens
for causal in (False, True):
    cz = "causal" if causal else "plain"
    for i, (T, kl) in enumerate(((40, (1, 16, 17)), (40, (32, 33, 39)), (40, (40, 39, 1)), (145, (129, 144, 145)), (321, (1, 320, 200)))):
        CASES.append(Case(f"klen-{cz}-{T}-{i}", f"attn_fwd_kernel<0,0,0> key_len + attn_bwd_kernel<0,0,{int(causal)},{_nt(T)}>", "ex",
                          3, 2, T, causal=causal, key_len=kl, pad=PAD, chained=(i == 1)))
# rectangular cross-attention, separate Q and [K | V] tensors, leading dimensions wider than the rows: Tq = 1, Tq > Tk, and
# max(tq, tk) = 128 | 129 decided by either side
for tq, tk, kl in ((1, 50, None), (1, 257, (257, 200, 1)), (77, 257, (256, 257, 17)), (257, 77, None), (35, 128, None), (35, 129, None),
                   (128, 35, (35, 34, 33)), (129, 35, None), (50, 1, None), (16, 512, None)):
    CASES.append(Case(f"cross-{tq}x{tk}", f"attn_fwd_kernel<0,0,0> NL{_nl(tk)} + attn_bwd_kernel<0,0,0,{_nt(max(tq, tk))}>", "ex",
                      3, 2, tq, tk, key_len=kl, pad=PAD, chained=(tq, tk) == (77, 257)))
# packed rows: the causal / plain self-attention of the text tower, and the general form with packed queries (K / V packed or dense
# with key_len), dropout on; item lengths 1, 16, 17, a middle value, the maximum
for causal in (False, True):
    cz = "causal" if causal else "plain"
    CASES.append(Case(f"packed-{cz}-77", f"attn_fwd_kernel<0,0,0> row_off + attn_bwd_kernel<0,0,{int(causal)},384>", "packed",
                      5, 2, 77, causal=causal, lens=(1, 16, 17, 40, 77), chained=True))
    CASES.append(Case(f"packed-{cz}-145", f"attn_fwd_kernel<0,0,0> row_off + attn_bwd_kernel<0,0,{int(causal)},512>", "packed",
                      3, 2, 145, causal=causal, lens=(1, 145, 17)))
for kvp in (1, 0):
    for p in (0.0, 0.1):
        CASES.append(Case(f"rows-kv{kvp}-drop{int(p * 10)}", f"attn_fwd_kernel<0,{int(p > 0)},0> q_row_off + attn_bwd_kernel<0,{int(p > 0)},0,384>",
                          "rows", 5, 2, 35, 35 if kvp else 50, lens=(1, 16, 17, 23, 35), kv_packed=kvp,
                          key_len=None if kvp else (50, 1, 17, 33, 49), drop_p=p, pad=PAD, chained=(p > 0)))
CASES.append(Case("rows-kv1-drop1-145", "attn_fwd_kernel<0,1,0> q_row_off + attn_bwd_kernel<0,1,0,512>", "rows", 3, 2, 145, 145,
                  lens=(145, 1, 130), kv_packed=1, drop_p=0.1, pad=PAD))
# dropout through the general form: plain and causal, <= 128 and above, with key_len
for T, causal, kl in ((50, False, None), (145, False, None), (77, True, None), (145, True, None), (50, False, (1, 33, 49)),
                      (129, True, (129, 17, 128))):
    cz = "causal" if causal else "plain"
    CASES.append(Case(f"drop-{cz}-{T}{'-klen' if kl else ''}", f"attn_fwd_kernel<0,1,0> + attn_bwd_kernel<0,1,{int(causal)},{_nt(T)}>", "ex",
                      3, 2, T, causal=causal, key_len=kl, drop_p=0.1, pad=PAD, chained=(T == 77)))
# relative bias (scale 1), with and without dropout; drel judged in every one
for T in (16, 50, 129, 334):
    for p in (0.0, 0.1):
        CASES.append(Case(f"rel-{T}-drop{int(p * 10)}", f"attn_fwd_kernel<1,{int(p > 0)},0> + attn_bwd_kernel<1,{int(p > 0)},0,{_nt(T)}>", "rel",
                          2, 3 if T < 334 else 2, T, drop_p=p, nbuckets=32, chained=(T == 50)))
# the pair-tile backward: taken (nvl = 1 and 7 at the 224 padding, 1 at 288), the first sizes it refuses (the general kernel
# runs), wider leading dimensions, more (item, head) pairs than compute units (the persistent walk) and fewer
for T in (193, 197, 199, 257):
    CASES.append(Case(f"pair-{T}", f"attn_fwd_kernel<0,0,0> + attn_bwd_pair_kernel<{224 if T < 224 else 288}>", "qkv", 2, 3, T,
                      chained=(T == 199)))
for T in (192, 200, 256, 258):
    CASES.append(Case(f"pair-refused-{T}", "attn_fwd_kernel<0,0,0> + attn_bwd_kernel<0,0,0,512>", "qkv", 2, 2, T))
CASES.append(Case("pair-197-ld", "attn_fwd_kernel<0,0,0> + attn_bwd_pair_kernel<224> dq_ld / dkv_ld", "ex", 2, 2, 197, pad=PAD))
CASES.append(Case("pair-257-ld", "attn_fwd_kernel<0,0,0> + attn_bwd_pair_kernel<288> dq_ld / dkv_ld", "ex", 2, 2, 257, pad=PAD))
CASES.append(Case("pair-193-walk", "attn_fwd_kernel<0,0,0> + attn_bwd_pair_kernel<224> persistent walk", "qkv", 65, 4, 193))
# the streaming kernels: one chunk past 512, whole and partial last chunks, the largest size
for T in (513, 576, 577, 641, 1023, 1024):
    CASES.append(Case(f"long-{T}", "attn_long_fwd_kernel<0> + attn_long_dkdv_kernel + attn_long_dq_kernel", "qkv", 2, 2, T,
                      chained=(T == 577)))
    CASES.append(Case(f"long-f16-{T}", "attn_long_fwd_kernel<1>", "f16", 2, 2, T))

_names = [c.name for c in CASES]
assert len(set(_names)) == len(_names), [n for n in _names if _names.count(n) > 1]
for _c in CASES:          # the contract: no empty item, no key_len below 1
    assert _c.lens is None or min(_c.lens) >= 1
    assert _c.key_len is None or min(_c.key_len) >= 1
    if "pair_kernel" in _c.path:
        assert _pair_takes(_c.tq) and _c.tq == _c.tk
    elif _c.api == "qkv" and _c.tq <= 512 and not _c.causal:
        assert not _pair_takes(_c.tq)


# ------------------------------------------------------------------------------------------------------------- guarded storage
def _lib():
    from uniir_amd import _lib
    return _lib.load()


def _stream():
    from uniir_amd import ops
    return ops._stream()


class Buf:
    """a [rows][cols] view of pitch ld with GUARD rows behind it; every element outside the view holds the NaN pattern"""

    def __init__(self, rows, cols, ld, dtype):
        assert ld >= cols
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        self.ibits = {2: torch.int16, 4: torch.int32}[dtype.itemsize]
        self.flat = torch.empty((rows + GUARD) * ld, dtype=dtype, device=DEV)
        pat = NAN16[dtype] if dtype.itemsize == 2 else NAN32
        self.flat.view(self.ibits).fill_(pat - (1 << 16) if (dtype.itemsize == 2 and pat >= 1 << 15) else pat)
        self.view = self.flat.as_strided((rows, cols), (ld, 1))

    def ptr(self, col=0):
        return C.c_void_p(self.flat.data_ptr() + col * self.dtype.itemsize)

    def bits(self):
        return self.flat.view(self.ibits)

    def outside(self):
        m = torch.ones(self.flat.numel(), dtype=torch.bool, device=DEV)
        m.as_strided((self.rows, self.cols), (self.ld, 1)).fill_(False)
        return m


def _untouched(name, buf, before, extra_mask=None):
    mask = buf.outside()
    if extra_mask is not None:
        mask = mask | extra_mask
    now = buf.bits()
    if not torch.equal(now[mask], before[mask]):
        raise AssertionError(f"{name}: {int((now[mask] != before[mask]).sum())} elements changed outside the logical extent")


def _i32(xs):
    return torch.tensor(list(xs), dtype=torch.int32, device=DEV)


def _dropf(p):
    def f(count):
        out = torch.empty(count, dtype=torch.float32, device=DEV)
        rc = _lib().uniir_dropout_mask(C.c_void_p(out.data_ptr()), count, C.c_float(p), DROP_SEED, _stream())
        assert rc == 0
        return out
    return f


class Run:
    """the buffers of one case and its calls"""

    def __init__(self, c, items, dense=False):
        """dense: the padded twin of a packed case (uniir_attention_*_ex on the items' full tq / tk rows with key_len = the lengths)"""
        self.c, self.items, self.dense = c, items, dense
        H = c.heads
        self.W = W = H * 64
        self.api = "ex" if dense else c.api
        self.fused = self.api in ("qkv", "f16", "packed", "rel")
        packed_q = c.lens is not None and not dense
        packed_k = packed_q and (c.api == "packed" or c.kv_packed)
        self.qlen = [it.Tq if packed_q else c.tq for it in items]
        self.klen = [it.Tk if packed_k else c.tk for it in items]
        self.q0 = [sum(self.qlen[:m]) for m in range(c.batch + 1)]
        self.k0 = [sum(self.klen[:m]) for m in range(c.batch + 1)]
        self.row_off = _i32(self.q0) if packed_q else None
        if dense:
            self.key_len = _i32([it.twin_key_len for it in items])
        else:
            self.key_len = None if c.key_len is None else _i32(c.key_len)
        pad = c.pad
        nq, nk = self.q0[-1], self.k0[-1]
        if self.fused:
            assert nq == nk
            self.X = Buf(nq, 3 * W, 3 * W, c.dtype)
            self.q_ld = self.kv_ld = self.dq_ld = self.dkv_ld = 3 * W
            self.out_ld = W
        else:
            self.Q = Buf(nq, W, W + pad, c.dtype)
            self.KV = Buf(nk, 2 * W, 2 * W + pad, c.dtype)
            self.q_ld, self.kv_ld = W + pad, 2 * W + pad
            self.out_ld, self.dq_ld, self.dkv_ld = W + pad + 8, W + pad + 16, 2 * W + pad + 24
        for m, it in enumerate(items):
            q, k, v, _ = it.twin
            lq, lk = self.qlen[m], self.klen[m]
            if self.fused:
                rows = self.X.view[self.q0[m]:self.q0[m] + lq]
                rows[:, :W], rows[:, W:2 * W], rows[:, 2 * W:] = q[:lq].reshape(lq, W), k[:lk].reshape(lk, W), v[:lk].reshape(lk, W)
            else:
                self.Q.view[self.q0[m]:self.q0[m] + lq] = q[:lq].reshape(lq, W)
                rows = self.KV.view[self.k0[m]:self.k0[m] + lk]
                rows[:, :W], rows[:, W:] = k[:lk].reshape(lk, W), v[:lk].reshape(lk, W)
        self.nq, self.nk = nq, nk

    # -- pointers of the operands
    def _qkv(self):
        if self.fused:
            return self.X.ptr(0), self.X.ptr(self.W), self.X.ptr(2 * self.W)
        return self.Q.ptr(0), self.KV.ptr(0), self.KV.ptr(self.W)

    def live_lse(self):
        """bool [batch][H][tq]: the lse entries the call writes"""
        c = self.c
        m = torch.zeros(c.batch, c.heads, c.tq, dtype=torch.bool, device=DEV)
        for i, l in enumerate(self.qlen):
            m[i, :, :l] = True
        return m

    def forward(self):
        c, lib, W = self.c, _lib(), self.W
        self.out = Buf(self.nq, W, self.out_ld, c.dtype)
        self.lse = Buf(1, c.batch * c.heads * c.tq, c.batch * c.heads * c.tq + TAIL, torch.float32)
        before = {"out": self.out.bits().clone(), "lse": self.lse.bits().clone()}
        q, k, v = self._qkv()
        st = _stream()
        kl = None if self.key_len is None else C.c_void_p(self.key_len.data_ptr())
        ro = None if self.row_off is None else C.c_void_p(self.row_off.data_ptr())
        if self.api == "qkv":
            rc = lib.uniir_attention_fwd(q, self.out.ptr(), self.lse.ptr(), c.batch, c.tq, c.heads, int(c.causal), st)
        elif self.api == "f16":
            rc = lib.uniir_attention_fwd_f16(q, self.out.ptr(), self.lse.ptr(), None, c.batch, c.tq, c.heads, int(c.causal), st)
        elif self.api == "packed":
            rc = lib.uniir_attention_fwd_packed(q, self.out.ptr(), self.lse.ptr(), ro, c.batch, c.tq, c.heads, int(c.causal), st)
        elif self.api == "ex":
            rc = lib.uniir_attention_fwd_ex(q, self.q_ld, k, v, self.kv_ld, self.out.ptr(), self.out_ld, self.lse.ptr(), kl, c.batch, c.tq,
                                            c.tk, c.heads, int(c.causal), c.drop_p, DROP_SEED, st)
        elif self.api == "rows":
            rc = lib.uniir_attention_fwd_rows(q, self.q_ld, k, v, self.kv_ld, self.out.ptr(), self.out_ld, self.lse.ptr(), ro, c.kv_packed,
                                              kl, c.batch, c.tq, c.tk, c.heads, c.drop_p, DROP_SEED, st)
        else:
            it = self.items[0]
            self.emb, self.bucket = it.rel_emb.contiguous(), it.rel_bucket.contiguous()
            rc = lib.uniir_attention_rel_fwd(q, self.out.ptr(), self.lse.ptr(), C.c_void_p(self.emb.data_ptr()),
                                             C.c_void_p(self.bucket.data_ptr()), c.nbuckets, 1.0, c.batch, c.tq, c.heads, c.drop_p,
                                             DROP_SEED, st)
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        _untouched(f"{c.name} out", self.out, before["out"])
        dead = torch.ones(self.lse.flat.numel(), dtype=torch.bool, device=DEV)
        dead[:c.batch * c.heads * c.tq] = ~self.live_lse().flatten()
        _untouched(f"{c.name} lse", self.lse, before["lse"], dead & ~self.lse.outside())
        return self.item_outputs_fwd()

    def item_outputs_fwd(self):
        c = self.c
        lse = self.lse.view[0].view(c.batch, c.heads, c.tq)
        return [{"out": self.out.view[self.q0[m]:self.q0[m] + self.qlen[m]].reshape(self.qlen[m], c.heads, 64),
                 "lse": lse[m, :, :self.qlen[m]]} for m in range(c.batch)]

    def backward(self, out_in, lse_in, dout=None):
        """out_in / lse_in per item ([Tq][H][64] 16-bit, [H][Tq] fp32); dead lse entries hold NaN"""
        c, lib, W = self.c, _lib(), self.W
        O, dO = Buf(self.nq, W, self.out_ld, c.dtype), Buf(self.nq, W, self.out_ld, c.dtype)
        L = Buf(1, c.batch * c.heads * c.tq, c.batch * c.heads * c.tq + TAIL, torch.float32)
        lview = L.view[0].view(c.batch, c.heads, c.tq)
        for m, it in enumerate(self.items):
            lq = self.qlen[m]
            O.view[self.q0[m]:self.q0[m] + lq] = out_in[m].reshape(lq, W)
            dO.view[self.q0[m]:self.q0[m] + lq] = (it.twin[3][:lq] if dout is None else dout[m]).reshape(lq, W)
            lview[m, :, :lq] = lse_in[m]
        if self.fused:
            self.dX = Buf(self.nq, 3 * W, 3 * W, c.dtype)
            dq, dk, dv = self.dX.ptr(0), self.dX.ptr(W), self.dX.ptr(2 * W)
            outs = {"dqkv": self.dX}
        else:
            self.dQ, self.dKV = Buf(self.nq, W, self.dq_ld, c.dtype), Buf(self.nk, 2 * W, self.dkv_ld, c.dtype)
            dq, dk, dv = self.dQ.ptr(0), self.dKV.ptr(0), self.dKV.ptr(W)
            outs = {"dq": self.dQ, "dkv": self.dKV}
        if self.api == "rel":
            self.drel = Buf(1, c.nbuckets * c.heads, c.nbuckets * c.heads + TAIL, torch.float32)
            self.drel.view.zero_()
            outs["drel"] = self.drel
        before = {k: b.bits().clone() for k, b in outs.items()}
        q, k, v = self._qkv()
        st = _stream()
        kl = None if self.key_len is None else C.c_void_p(self.key_len.data_ptr())
        ro = None if self.row_off is None else C.c_void_p(self.row_off.data_ptr())
        if self.api == "qkv":
            rc = lib.uniir_attention_bwd(q, O.ptr(), dO.ptr(), L.ptr(), dq, c.batch, c.tq, c.heads, int(c.causal), st)
        elif self.api == "packed":
            rc = lib.uniir_attention_bwd_packed(q, O.ptr(), dO.ptr(), L.ptr(), dq, ro, c.batch, c.tq, c.heads, int(c.causal), st)
        elif self.api == "ex":
            rc = lib.uniir_attention_bwd_ex(q, self.q_ld, k, v, self.kv_ld, O.ptr(), dO.ptr(), self.out_ld, L.ptr(), kl, dq, self.dq_ld, dk,
                                            dv, self.dkv_ld, c.batch, c.tq, c.tk, c.heads, int(c.causal), c.drop_p, DROP_SEED, st)
        elif self.api == "rows":
            rc = lib.uniir_attention_bwd_rows(q, self.q_ld, k, v, self.kv_ld, O.ptr(), dO.ptr(), self.out_ld, L.ptr(), ro, c.kv_packed, kl,
                                              dq, self.dq_ld, dk, dv, self.dkv_ld, c.batch, c.tq, c.tk, c.heads, c.drop_p, DROP_SEED, st)
        else:
            rc = lib.uniir_attention_rel_bwd(q, O.ptr(), dO.ptr(), L.ptr(), dq, C.c_void_p(self.emb.data_ptr()),
                                             C.c_void_p(self.bucket.data_ptr()), c.nbuckets, 1.0, self.drel.ptr(), c.batch, c.tq, c.heads,
                                             c.drop_p, DROP_SEED, st)
        torch.cuda.synchronize()
        assert rc == 0, (c.name, rc)
        for name, b in outs.items():
            _untouched(f"{c.name} {name}", b, before[name])
        return self.item_outputs_bwd()

    def item_outputs_bwd(self):
        c, W, res = self.c, self.W, []
        for m in range(c.batch):
            lq, lk = self.qlen[m], self.klen[m]
            if self.fused:
                rows = self.dX.view[self.q0[m]:self.q0[m] + lq]
                d = {"dq": rows[:, :W], "dk": rows[:, W:2 * W], "dv": rows[:, 2 * W:]}
            else:
                kv = self.dKV.view[self.k0[m]:self.k0[m] + lk]
                d = {"dq": self.dQ.view[self.q0[m]:self.q0[m] + lq], "dk": kv[:, :W], "dv": kv[:, W:]}
            res.append({n: t.reshape(t.shape[0], c.heads, 64) for n, t in d.items()})
        return res


# ------------------------------------------------------------------------------------------------------------------ judging
def _judge(c, what, got_items, ref_items, ratios):
    """every output of every item inside its bound; ratios[name] collects the largest |got - ref| / bound"""
    for m, (got, ref) in enumerate(zip(got_items, ref_items)):
        for name, g in got.items():
            r, b = ref[name]
            why = R.compare(g, r, b, torch.float32 if name == "lse" else c.dtype)
            ratios[name] = max(ratios.get(name, 0.0), R.worst(g, r, b))
            assert why is None, f"{c.name} ({c.path}) {what} item {m} {name}: {why}"


def _masked_keys_zero(c, items, got_items):
    for m, (it, got) in enumerate(zip(items, got_items)):
        kv = it.kvalid
        if kv < it.Tk:
            for name in ("dk", "dv"):
                assert not bool(got[name][kv:].float().abs().any()), f"{c.name} item {m}: {name} of masked keys is not exactly zero"


def _drel(c, run, refs, ratios, what):
    ref = sum(r["drel"][0] for r in refs)
    mag = sum(r["drel_mag"] for r in refs)
    bound = sum(r["drel"][1] for r in refs) + 2.0 * (c.batch + 2) * R.EPS32 * mag
    got = run.drel.view[0].view(c.nbuckets, c.heads)
    why = R.compare(got, ref, bound, torch.float32)
    ratios["drel"] = max(ratios.get("drel", 0.0), R.worst(got, ref, bound))
    assert why is None, f"{c.name} ({c.path}) {what} drel: {why}"
    return got.clone()


def _round_ref(c, fref):
    """the reference forward results rounded to what a backward reads"""
    return [f["out"][0].to(c.dtype) for f in fref], [f["lse"][0].float() for f in fref]


def _bwd_refs(items, out_in, lse_in):
    refs = [it.bwd_ref(o, l) for it, o, l in zip(items, out_in, lse_in)]
    return refs, [{k: r[k] for k in ("dq", "dk", "dv")} for r in refs]


@pytest.fixture(autouse=True)
def _time_limit():
    faulthandler.dump_traceback_later(CASE_SECONDS, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _fmt(ratios):
    return " ".join(f"{k}={v:.3f}" for k, v in ratios.items())


@pytest.mark.parametrize("case", CASES, ids=_names)
def test_attention_path(case):
    c = case
    items = R.build_items(c, DEV, _dropf(c.drop_p) if c.drop_p > 0 else None)
    run = Run(c, items)
    got_f = run.forward()
    fref = [it.fwd_ref()[0] for it in items]
    ratios = {}
    _judge(c, "forward", got_f, fref, ratios)
    out_bits, lse_bits = run.out.bits().clone(), run.lse.bits().clone()
    run.forward()
    assert torch.equal(run.out.bits(), out_bits) and torch.equal(run.lse.bits(), lse_bits), f"{c.name}: the forward differs between two runs"
    print(f"\nOBS {c.name} [{c.path}] forward {_fmt(ratios)}")
    own = [{k: v.clone() for k, v in g.items()} for g in got_f]
    if c.bwd:
        out_in, lse_in = _round_ref(c, fref)
        for what, (o_in, l_in) in (("backward", (out_in, lse_in)), ("chained", ([g["out"] for g in own], [g["lse"] for g in own]))):
            if what == "chained" and not c.chained:
                continue
            ratios = {}
            got_b = run.backward(o_in, l_in)
            refs, dref = _bwd_refs(items, o_in, l_in)
            _judge(c, what, got_b, dref, ratios)
            _masked_keys_zero(c, items, got_b)
            bits = [b.bits().clone() for b in ((run.dX,) if run.fused else (run.dQ, run.dKV))]
            d1 = _drel(c, run, refs, ratios, what) if c.api == "rel" else None
            run.backward(o_in, l_in)
            for b, old in zip((run.dX,) if run.fused else (run.dQ, run.dKV), bits):
                assert torch.equal(b.bits(), old), f"{c.name}: the {what} differs between two runs"
            extra = ""
            if d1 is not None:
                d2 = run.drel.view[0].view(c.nbuckets, c.heads)
                extra = f" drel_repeat_diff={float((d1 - d2).abs().max()):.3g}"
            print(f"OBS {c.name} [{c.path}] {what} {_fmt(ratios)}{extra}")
    if c.lens is not None:
        _same_as_dense(c, items, run, own)


def _same_as_dense(c, items, run, own_f):
    """live rows of a packed call are bitwise those of the dense padded call (dout of the padding rows is zero there, as in the
    models; forward and backward chained on each call's own results)"""
    dense = Run(c, items, dense=True)
    got_f = dense.forward()
    for m, it in enumerate(items):
        for name in ("out", "lse"):
            d = got_f[m][name][:it.Tq] if name == "out" else got_f[m][name][:, :it.Tq]
            assert torch.equal(d, own_f[m][name]), f"{c.name} item {m}: {name} of the packed call differs from the dense call"
    if not c.bwd:
        return
    got_p = run.backward([g["out"] for g in own_f], [g["lse"] for g in own_f])
    got_p = [{k: v.clone() for k, v in g.items()} for g in got_p]
    got_d = dense.backward([g["out"] for g in got_f], [g["lse"] for g in got_f], dout=[it.twin[3] for it in items])
    for m, it in enumerate(items):
        for name, n in (("dq", it.Tq), ("dk", it.Tk), ("dv", it.Tk)):
            assert torch.equal(got_d[m][name][:n], got_p[m][name]), f"{c.name} item {m}: {name} of the packed call differs from the dense call"


# --------------------------------------------------------------------------------------------------------------- rejections
def _reject_args():
    """(name, entry point, expected code, argument list without the stream): calls the entry points refuse on the host.  Every
    pointer is a valid, aligned buffer unless the case is about it."""
    H, W = 2, 128
    big = torch.zeros(1100 * 3 * W + 64, dtype=BF, device=DEV)
    outb = torch.full((1100 * 3 * W + 64,), float("nan"), dtype=BF, device=DEV)
    lse = torch.full((4096,), float("nan"), dtype=torch.float32, device=DEV)
    ints = torch.ones(4200, dtype=torch.int32, device=DEV)
    emb = torch.zeros(128 * H, dtype=torch.float32, device=DEV)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)          # noqa: E731
    b, o, L, I, E = P(big), P(outb), P(lse), P(ints), P(emb)

    def ex(tq=16, tk=16, causal=0, q_ld=W, kv_ld=2 * W, out_ld=W, q=b, p=0.0):
        return [q, q_ld, b, b, kv_ld, o, out_ld, L, None, 1, tq, tk, H, causal, p, 1]

    def exb(tq=16, tk=16, causal=0, q_ld=W, dq_ld=W, dkv_ld=2 * W, dq=o, p=0.0):
        return [b, q_ld, b, b, 2 * W, b, b, W, L, None, dq, dq_ld, o, o, dkv_ld, 1, tq, tk, H, causal, p, 1]

    def rows(tq=16, tk=16, kvp=0, kl=None, out_ld=W, p=0.0):
        return [b, W, b, b, 2 * W, o, out_ld, L, I, kvp, kl, 1, tq, tk, H, p, 1]

    def rowsb(tq=16, tk=16, kvp=0, kl=None, dq_ld=W, p=0.0):
        return [b, W, b, b, 2 * W, b, b, W, L, I, kvp, kl, o, dq_ld, o, o, 2 * W, 1, tq, tk, H, p, 1]

    def rel(seq=16, nb=32, p=0.0):
        return [b, o, L, E, I, nb, 1.0, 1, seq, H, p, 1]

    def relb(seq=16, nb=32, p=0.0):
        return [b, b, b, L, o, E, I, nb, 1.0, E, 1, seq, H, p, 1]

    t = [
        ("ex-tq-513", "uniir_attention_fwd_ex", "ESHAPE", ex(tq=513, tk=16)),
        ("ex-tk-513", "uniir_attention_fwd_ex", "ESHAPE", ex(tq=16, tk=513)),
        ("exb-tq-513", "uniir_attention_bwd_ex", "ESHAPE", exb(tq=513)),
        ("exb-tk-513", "uniir_attention_bwd_ex", "ESHAPE", exb(tk=513)),
        ("rows-tq-513", "uniir_attention_fwd_rows", "ESHAPE", rows(tq=513, tk=513)),
        ("rowsb-tk-513", "uniir_attention_bwd_rows", "ESHAPE", rowsb(tk=513)),
        ("rel-513", "uniir_attention_rel_fwd", "ESHAPE", rel(seq=513)),
        ("relb-513", "uniir_attention_rel_bwd", "ESHAPE", relb(seq=513)),
        ("packed-513", "uniir_attention_fwd_packed", "ESHAPE", [b, o, L, I, 1, 513, H, 0]),
        ("packedb-513", "uniir_attention_bwd_packed", "ESHAPE", [b, b, b, L, o, I, 1, 513, H, 1]),
        ("ex-causal-rect", "uniir_attention_fwd_ex", "ESHAPE", ex(tq=16, tk=32, causal=1)),
        ("exb-causal-rect", "uniir_attention_bwd_ex", "ESHAPE", exb(tq=32, tk=16, causal=1)),
        ("fwd-causal-513", "uniir_attention_fwd", "ESHAPE", [b, o, L, 1, 513, H, 1]),
        ("bwd-causal-513", "uniir_attention_bwd", "ESHAPE", [b, b, b, L, o, 1, 513, H, 1]),
        ("fwd-1025", "uniir_attention_fwd", "ESHAPE", [b, o, L, 1, 1025, H, 0]),
        ("bwd-1025", "uniir_attention_bwd", "ESHAPE", [b, b, b, L, o, 1, 1025, H, 0]),
        ("ex-q_ld-132", "uniir_attention_fwd_ex", "EALIGN", ex(q_ld=W + 4)),
        ("ex-kv_ld-260", "uniir_attention_fwd_ex", "EALIGN", ex(kv_ld=2 * W + 4)),
        ("ex-out_ld-129", "uniir_attention_fwd_ex", "EALIGN", ex(out_ld=W + 1)),
        ("exb-dq_ld-132", "uniir_attention_bwd_ex", "EALIGN", exb(dq_ld=W + 4)),
        ("exb-dkv_ld-258", "uniir_attention_bwd_ex", "EALIGN", exb(dkv_ld=2 * W + 2)),
        ("rows-out_ld-132", "uniir_attention_fwd_rows", "EALIGN", rows(out_ld=W + 4)),
        ("rowsb-dq_ld-132", "uniir_attention_bwd_rows", "EALIGN", rowsb(dq_ld=W + 4)),
        ("ex-q-misaligned", "uniir_attention_fwd_ex", "EALIGN", ex(q=P(big, 8))),
        ("exb-dq-misaligned", "uniir_attention_bwd_ex", "EALIGN", exb(dq=P(outb, 2))),
        ("fwd-qkv-misaligned", "uniir_attention_fwd", "EALIGN", [P(big, 4), o, L, 1, 16, H, 0]),
        ("f16-out-misaligned", "uniir_attention_fwd_f16", "EALIGN", [b, P(outb, 8), L, None, 1, 16, H, 0]),
        ("ex-drop-1", "uniir_attention_fwd_ex", "EINVAL", ex(p=1.0)),
        ("ex-drop-neg", "uniir_attention_fwd_ex", "EINVAL", ex(p=-0.1)),
        ("exb-drop-1", "uniir_attention_bwd_ex", "EINVAL", exb(p=1.0)),
        ("rows-drop-1", "uniir_attention_fwd_rows", "EINVAL", rows(p=1.0)),
        ("rowsb-drop-neg", "uniir_attention_bwd_rows", "EINVAL", rowsb(p=-0.5)),
        ("rel-drop-1", "uniir_attention_rel_fwd", "EINVAL", rel(p=1.0)),
        ("relb-drop-1", "uniir_attention_rel_bwd", "EINVAL", relb(p=1.5)),
        ("rel-buckets-65", "uniir_attention_rel_fwd", "EINVAL", rel(nb=65)),
        ("relb-buckets-65", "uniir_attention_rel_bwd", "EINVAL", relb(nb=65)),
        ("rows-kvp-keylen", "uniir_attention_fwd_rows", "EINVAL", rows(kvp=1, kl=I)),
        ("rows-kvp-rect", "uniir_attention_fwd_rows", "EINVAL", rows(tq=16, tk=32, kvp=1)),
        ("rowsb-kvp-keylen", "uniir_attention_bwd_rows", "EINVAL", rowsb(kvp=1, kl=I)),
        ("rowsb-kvp-rect", "uniir_attention_bwd_rows", "EINVAL", rowsb(tq=32, tk=16, kvp=1)),
        ("f16-1025", "uniir_attention_fwd_f16", "ESHAPE", [b, o, L, None, 1, 1025, H, 0]),
        ("f16-causal-513", "uniir_attention_fwd_f16", "ESHAPE", [b, o, L, None, 1, 513, H, 1]),
        ("f16-packed-513", "uniir_attention_fwd_f16", "ESHAPE", [b, o, L, I, 1, 513, H, 0]),
    ]
    return t, (outb, lse)


def test_rejections():
    """the documented code, and nothing written"""
    table, (outb, lse) = _reject_args()
    lib = _lib()
    wrong = []
    for name, fn, code, args in table:
        rc = getattr(lib, fn)(*args, _stream())
        torch.cuda.synchronize()
        if rc != ERR[code]:
            wrong.append((name, fn, code, rc))
    assert not wrong, wrong
    assert bool(torch.isnan(outb).all()) and bool(torch.isnan(lse).all()), "a refused call wrote to an output"


# ------------------------------------------------------------------------------------------------- which kernels each case runs
def _expected_kernels(path):
    """the kernel names a case's path string stands for, as a profiler prints them: attn_fwd_kernel<0,1,0> -> attn_fwd_kernel<false, true, false>"""
    import re
    out = []
    for name, args in re.findall(r"(attn_\w+_kernel)(?:<([\d,]+)>)?", path):
        if not args:
            out.append(name)
            continue
        a = args.split(",")
        if name in ("attn_fwd_kernel", "attn_long_fwd_kernel"):
            a = ["true" if int(x) else "false" for x in a]
        elif name == "attn_bwd_kernel":
            a = ["true" if int(x) else "false" for x in a[:3]] + a[3:]
        out.append(f"{name}<{', '.join(a)}>")
    return out


def test_every_case_launches_its_paths_kernels():
    """every case once more under torch.profiler, without the references: the attention kernels it launches are those its path names
    (the pair kernel at the sizes ap_geom takes and the general one at the first sizes it refuses, 384 / 512 threads, ...)"""
    from torch.profiler import ProfilerActivity, profile
    found = {}
    for c in CASES:
        items = R.build_items(c, DEV, _dropf(c.drop_p) if c.drop_p > 0 else None)
        run = Run(c, items)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            got = run.forward()
            if c.bwd:
                run.backward([g["out"] for g in got], [g["lse"] for g in got])
            torch.cuda.synchronize()
        names = sorted({e.name.replace("void ", "").split("(")[0] for e in prof.events()
                        if e.device_type == torch.autograd.DeviceType.CUDA and "attn_" in e.name})
        found[c.name] = (c.path, names)
        del run, items
    for name, (path, kn) in found.items():
        print(f"KERNELS {name:28s} {'  '.join(kn)}")
    if not any(kn for _, kn in found.values()):
        pytest.skip("the profiler saw none of the library's kernels")
    wrong = [(name, path, kn) for name, (path, kn) in found.items() if sorted(_expected_kernels(path)) != kn]
    assert not wrong, wrong
