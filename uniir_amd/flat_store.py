"""The parameter storage of every model here (CLIP, the BLIP online and momentum encoders, the CLIP_FF T5 stack): one flat fp32
master buffer, an optional flat fp32 gradient buffer and a bf16 shadow for an ordered list of named tensors.  The kernels and the C
tower read the tensors through raw offsets into these buffers; the nn.Parameters a model exposes are views of them (adopt())."""
import math

import torch

from . import ops

ALIGN = 64  # elements; every tensor starts on a 256-B boundary of the flat buffers


def padded(numel):
    return (numel + ALIGN - 1) // ALIGN * ALIGN


class FlatStore:
    """p32 fp32 [total] (master weights), g32 fp32 [total] (gradients; None without), w16_buf bf16 [total] (shadow of
    p32, refresh_shadow()); tensor `name` occupies [off[name], off[name] + numel) of each, in the order it was given.
    The named views are p(name) (fp32), w16(name) and grad_view(name); w16h(name) is w16's twin in the optional fp16 shadow
    (h16_buf: the forward-only fp16 path, built on first use)."""

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
        # the optional fp16 shadow (w16h()): `total` halves in the same layout, allocated and filled on first use, filled again on
        # the next use once marked stale -- by refresh_shadow(), and by mark_half_stale() for writers that go past this class (the
        # fused AdamW and EMA kernels write p32 and w16_buf themselves).  A store that never asks for it allocates nothing.
        self.h16_buf = None
        self.half_stale = True

    @classmethod
    def adopt(cls, named, device, with_grad=True, frozen=()):
        """a store over the (name, parameter) pairs `named`, in that order: the values are copied in and every parameter becomes a
        view of the master buffer, its .grad a view of the gradient buffer (except the `frozen` names, which keep no gradient)"""
        st = cls([(n, p.shape) for n, p in named], device, with_grad)
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

    def ptr(self, buf, name):
        """device address of `name` inside `buf` (one of this store's buffers, or another buffer of `total` elements in the same
        layout, e.g. CLIP's fp16 shadow)"""
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
        ops.call("uniir_cast_f32_to_bf16", self.p32, self.w16_buf, self.total)
        self.half_stale = True

    def mark_half_stale(self):
        """the master weights moved without refresh_shadow() (a kernel that writes p32 and the bf16 shadow itself)"""
        self.half_stale = True

    def half_shadow(self):
        """the fp16 shadow of p32, up to date: one cast of the whole buffer on first use and after every event that marked it stale"""
        if self.h16_buf is None:
            self.h16_buf = torch.empty(self.total, device=self.dev, dtype=torch.float16)
            self.half_stale = True
        if self.half_stale:
            ops.call("uniir_cast_f32_to_f16", self.p32, self.h16_buf, self.total)
            self.half_stale = False
        return self.h16_buf

    def zero_grad(self, named, frozen=()):
        """one memset of the gradient buffer; a parameter whose .grad was replaced gets its view back"""
        self.g32.zero_()
        for n, p in named:
            if n not in frozen and (p.grad is None or p.grad.data_ptr() != self.ptr(self.g32, n)):
                p.grad = self.grad_view(n)
