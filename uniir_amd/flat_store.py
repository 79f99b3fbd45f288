"""The parameter storage of every model here (CLIP, the BLIP online and momentum encoders, the CLIP_FF T5 stack): one flat fp32
master buffer, an optional flat fp32 gradient buffer and a bf16 shadow for an ordered list of named tensors.  The kernels and the C
tower read the tensors through raw offsets into these buffers; the nn.Parameters a model exposes are views of them (adopt()).
Every 16-bit copy of the masters lives here too, under one rule for "the copies follow the masters" (FlatStore)."""
import math

import torch

from . import ops

ALIGN = 64  # elements; every tensor starts on a 256-B boundary of the flat buffers


def padded(numel):
    return (numel + ALIGN - 1) // ALIGN * ALIGN


def patch_kpad(P):
    """leading dimension of a [width, 3 P P] patch-embedding weight re-laid out for the patchify GEMM: 3 P P up to whole 64s"""
    return (3 * P * P + 63) // 64 * 64


class _Padded:
    """the [rows, ld] copies of one [rows, cols] tensor (FlatStore.add_padded): bf16, its fp16 twin (None until the store's fp16
    shadow exists) and, in a store with gradients, the fp32 scratch a weight-gradient GEMM writes before uniir_unpad_add"""

    def __init__(self, rows, cols, ld, dev, with_grad):
        self.rows, self.cols, self.ld = rows, cols, ld
        self.w16 = torch.zeros(rows, ld, device=dev, dtype=torch.bfloat16)
        self.h16 = None
        self.g32 = torch.zeros(rows, ld, device=dev, dtype=torch.float32) if with_grad else None


class FlatStore:
    """p32 fp32 [total] (master weights), g32 fp32 [total] (gradients; None without), w16_buf bf16 [total] (shadow of
    p32, refresh_shadow()); tensor `name` occupies [off[name], off[name] + numel) of each, in the order it was given.
    The named views are p(name) (fp32), w16(name) and grad_view(name); w16h(name) is w16's twin in the optional fp16 shadow
    (h16_buf: the forward-only fp16 path, built on first use).  A tensor registered with add_padded() also has row-padded copies:
    padded16(name), padded16h(name) and padded_grad(name) stand beside w16 / w16h / grad_view.
    What moves the masters tells the store so, in one call: refresh_shadow() (or sync(), which finds out by itself) after torch wrote
    them, kernel_wrote() after a kernel that wrote p32 and w16_buf.  fp16 is never touched before half_shadow() asks for it."""

    def __init__(self, named_shapes, device, with_grad=True):
        self.off, self.shapes, cur = {}, {}, 0
        for n, shp in named_shapes:
            self.off[n], self.shapes[n] = cur, tuple(shp)
            cur += padded(math.prod(shp))
        self.total = cur
        self.p32 = torch.zeros(cur, device=device, dtype=torch.float32)
        self.g32 = torch.zeros(cur, device=device, dtype=torch.float32) if with_grad else None
        self.w16_buf = torch.empty(cur, device=device, dtype=torch.bfloat16)
        self.dev = self.p32.device
        # the optional fp16 shadow (w16h()): `total` halves in the same layout, allocated on first use and from then on filled IN PLACE
        # (raw pointers into it stay valid: CLIP.tower_desc caches them) on the next use after refresh_shadow() or kernel_wrote()
        # marked it stale.  A store that never asks for it allocates nothing.
        self.h16_buf = None
        self.half_stale = True
        self._pads = {}               # name -> _Padded (add_padded)
        self._versioned = []          # the adopted parameters whose torch-side writes sync() watches
        self._version = None          # their version sum at the last refresh_shadow()

    @classmethod
    def adopt(cls, named, device, with_grad=True, frozen=(), unversioned=()):
        """a store over the (name, parameter) pairs `named`, in that order: the values are copied in and every parameter becomes a
        view of the master buffer, its .grad a view of the gradient buffer (except the `frozen` names, which keep no gradient).
        sync() watches the parameters' versions, except the `unversioned` names (a tensor that no shadow is read of and that is
        written in place every step, BLIP's temp: it would make every sync() a refresh)"""
        st = cls([(n, p.shape) for n, p in named], device, with_grad)
        st._versioned = [p for n, p in named if n not in unversioned]
        for n, p in named:
            view = st.p(n)
            view.copy_(p.data.float())
            p.data = view
            if with_grad and n not in frozen:
                p.grad = st.grad_view(n)
        return st

    def holds(self, named):
        """True while every (name, parameter) still is the view adopt() made (.to(), a torch-side re-assignment of .data, ... end it)"""
        return all(p.device == self.dev and p.data_ptr() == self.ptr(self.p32, n) for n, p in named)

    def __getitem__(self, key):
        """store["p32"] / ["g32"] / ["w16"] (a whole buffer), ["off"] / ["shapes"] (the layout): the keys of the dict CLIP kept
        before this class, which bench.py and the tests read through CLIP._flat"""
        return {"p32": self.p32, "g32": self.g32, "w16": self.w16_buf, "off": self.off, "shapes": self.shapes}[key]

    # ---- named views and pointers --------------------------------------------------------------------------------
    def _view(self, buf, name, shape=None):
        shape = shape or self.shapes[name]
        o = self.off[name]
        return buf[o:o + math.prod(shape)].view(shape)

    def p(self, name, shape=None):
        """fp32 view of `name`; a larger `shape` spans the tensors that follow it (e.g. adjacent q / k / v weights as one)"""
        return self._view(self.p32, name, shape)

    def w16(self, name, shape=None):
        return self._view(self.w16_buf, name, shape)

    def w16h(self, name, shape=None):
        """fp16 view of `name` (same offsets and spans as w16) in the fp16 shadow, which is built or rebuilt here when it is stale"""
        return self._view(self.half_shadow(), name, shape)

    def grad_view(self, name, shape=None):
        return self._view(self.g32, name, shape)

    def add_padded(self, name, rows, cols, ld):
        """registers tensor `name`, read as [rows, cols], for row-padded [rows, ld] copies (zeros from column `cols` on: the
        patch-embedding weight as the patchify GEMM reads it).  Allocates the bf16 copy and, with gradients, the fp32 scratch;
        launches nothing: the copies are filled by the next refresh_shadow() / kernel_wrote()"""
        if rows * cols != math.prod(self.shapes[name]) or ld < cols:
            raise ValueError(f"add_padded: {name} {self.shapes[name]} as [{rows}, {cols}] with leading dimension {ld}")
        self._pads[name] = _Padded(rows, cols, ld, self.dev, self.g32 is not None)
        self.half_stale = True

    def padded16(self, name):
        """bf16 [rows, ld] copy of `name`"""
        return self._pads[name].w16

    def padded16h(self, name):
        """fp16 twin of padded16(name), brought up to date with the fp16 shadow (half_shadow())"""
        self.half_shadow()
        return self._pads[name].h16

    def padded_grad(self, name):
        """fp32 [rows, ld] scratch for the weight gradient of `name` in the padded layout (the caller zeroes, fills and unpads it)"""
        return self._pads[name].g32

    def ptr(self, buf, name):
        """device address of `name` inside `buf` (one of this store's buffers, or another buffer of `total` elements in the same
        layout, e.g. the optimizer's moments)"""
        return buf.data_ptr() + buf.element_size() * self.off[name]

    def span(self, names):
        """[lo, hi) covered by the tensors `names`, which must be adjacent (one range of the bucketed gradient all-reduce)"""
        lo = min(self.off[n] for n in names)
        hi = max(self.off[n] + padded(math.prod(self.shapes[n])) for n in names)
        if hi - lo != sum(padded(math.prod(self.shapes[n])) for n in names):
            raise RuntimeError(f"flat layout: {names} are not adjacent")
        return lo, hi

    def ranges(self, group_of):
        """the optimizer's launches over this store: (lo, hi, group) of every maximal run of consecutive tensors with one param group
        group_of(name); tensors whose group is None (frozen) are left out"""
        out = []
        for n, lo in self.off.items():
            gi, hi = group_of(n), lo + padded(math.prod(self.shapes[n]))
            if gi is None:
                continue
            if out and out[-1][1] == lo and out[-1][2] == gi:
                out[-1] = (out[-1][0], hi, gi)
            else:
                out.append((lo, hi, gi))
        return out

    # ---- device work ---------------------------------------------------------------------------------------------
    def refresh_shadow(self):
        """the masters moved on the torch side: one bf16 cast of the whole buffer, then everything kernel_wrote() does"""
        ops.call("uniir_cast_f32_to_bf16", self.p32, self.w16_buf, self.total)
        self.kernel_wrote()
        self._version = self._version_sum()

    def kernel_wrote(self):
        """the masters moved under a kernel that wrote p32 and the bf16 shadow itself (fused AdamW, EMA): the padded bf16 copies
        are not part of that shadow and are re-padded here, one launch per registered tensor; the fp16 copies go stale"""
        for name, pad in self._pads.items():
            ops.call("uniir_cast_pad_rows", self.p(name), pad.w16, pad.rows, pad.cols, pad.ld)
        self.half_stale = True

    def _version_sum(self):
        # torch-side writes (load_state_dict, in-place edits) bump these; a kernel's writes do not, and end in kernel_wrote()
        return sum(p._version for p in self._versioned)

    def sync(self):
        """refresh_shadow() if an adopted parameter was written on the torch side since the last one (or there was none yet)"""
        if self._version != self._version_sum():
            self.refresh_shadow()

    def half_shadow(self):
        """the fp16 shadow of p32, up to date, and with it the fp16 twins of the padded copies: one cast of the whole buffer and one
        pad per registered tensor, on first use and after every event that marked fp16 stale"""
        if self.h16_buf is None:
            self.h16_buf = torch.empty(self.total, device=self.dev, dtype=torch.float16)
            self.half_stale = True
        if self.half_stale:
            ops.call("uniir_cast_f32_to_f16", self.p32, self.h16_buf, self.total)
            for name, pad in self._pads.items():
                if pad.h16 is None:
                    pad.h16 = torch.zeros_like(pad.w16, dtype=torch.float16)
                ops.call("uniir_cast_pad_rows_f16", self.p(name), pad.h16, pad.rows, pad.cols, pad.ld)
            self.half_stale = False
        return self.h16_buf

    def half_bytes(self):
        """bytes the fp16 copies hold, padded twins included: 0 for a store that never asked for fp16"""
        return sum(t.numel() * 2 for t in [self.h16_buf] + [pad.h16 for pad in self._pads.values()] if t is not None)

    def zero_grad(self, named, frozen=()):
        """one memset of the gradient buffer; a parameter whose .grad was replaced gets its view back"""
        self.g32.zero_()
        for n, p in named:
            if n not in frozen and (p.grad is None or p.grad.data_ptr() != self.ptr(self.g32, n)):
                p.grad = self.grad_view(n)
