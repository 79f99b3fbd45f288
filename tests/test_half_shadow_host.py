"""Host-side bookkeeping of the forward-only fp16 path (no device): FlatStore's optional fp16 shadow, the 16-bit type that the ops
wrappers take from their operands, and the checks of the three fp16 glue entry points (a refused call returns before any HIP call)."""
import ctypes as C

import pytest
import torch

SHAPES = [("a.weight", (6, 10)), ("a.bias", (6,)), ("q.weight", (8, 8)), ("k.weight", (8, 8)), ("v.weight", (8, 8)), ("tail", (3, 5, 7))]


@pytest.fixture
def store(monkeypatch):
    """a FlatStore on the CPU whose device casts are recorded instead of launched"""
    from uniir_amd import flat_store
    calls = []
    monkeypatch.setattr(flat_store.ops, "call", lambda name, *a: calls.append((name,) + a))
    st = flat_store.FlatStore(SHAPES, "cpu")
    st.calls = calls
    return st


def _casts(st, name):
    return [c for c in st.calls if c[0] == name]


def test_nothing_is_allocated_until_the_fp16_shadow_is_asked_for(store):
    assert store.h16_buf is None
    store.refresh_shadow()
    store.kernel_wrote()
    store.w16("a.weight")
    store.p("q.weight", (24, 8))
    assert store.h16_buf is None and not _casts(store, "uniir_cast_f32_to_f16")
    assert [c[0] for c in store.calls] == ["uniir_cast_f32_to_bf16"]


def test_w16h_mirrors_w16_for_plain_and_spanning_shapes(store):
    for name, shape in [(n, None) for n, _ in SHAPES] + [("q.weight", (24, 8)), ("a.weight", (60,)), ("tail", (105,))]:
        h, b = store.w16h(name, shape), store.w16(name, shape)
        assert h.dtype == torch.float16 and b.dtype == torch.bfloat16
        assert h.shape == b.shape == torch.Size(shape or dict(SHAPES)[name])
        assert h.storage_offset() == b.storage_offset() == store.off[name]
        assert h.untyped_storage().data_ptr() == store.h16_buf.untyped_storage().data_ptr()
        assert store.ptr(store.h16_buf, name) - store.h16_buf.data_ptr() == store.ptr(store.w16_buf, name) - store.w16_buf.data_ptr()
    assert store.h16_buf.numel() == store.total == store.w16_buf.numel()


def test_the_shadow_is_cast_on_first_use_and_again_only_once_stale(store):
    f16 = "uniir_cast_f32_to_f16"
    store.w16h("a.weight")
    assert len(_casts(store, f16)) == 1
    name, src, dst, count = _casts(store, f16)[0]
    assert src is store.p32 and dst is store.h16_buf and count == store.total          # one cast of the whole buffer
    store.w16h("q.weight", (24, 8))
    store.half_shadow()
    assert len(_casts(store, f16)) == 1 and store.half_stale is False          # fresh: no second cast
    buf = store.h16_buf
    store.refresh_shadow()          # the event that refreshes the bf16 shadow marks the fp16 one ...
    assert store.half_stale is True and len(_casts(store, f16)) == 1          # ... and casts nothing by itself
    store.w16h("tail")
    assert len(_casts(store, f16)) == 2 and store.half_stale is False and store.h16_buf is buf          # rebuilt in place
    store.kernel_wrote()          # a writer that goes past the class (fused AdamW, EMA)
    assert store.half_stale is True
    store.half_shadow()
    store.half_shadow()
    assert len(_casts(store, f16)) == 3


def test_fp16_operands_with_a_causal_mask_dropout_or_mixed_types_are_value_errors():
    from uniir_amd import ops
    W = 128
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)
    b = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)
    q, kv = h(8, W), h(8, 2 * W)
    with pytest.raises(ValueError):
        ops.attention_fwd_ex(q, W, kv, kv[:, W:], 2 * W, 2, 4, 4, 2, causal=True)
    with pytest.raises(ValueError):
        ops.attention_fwd_ex(q, W, kv, kv[:, W:], 2 * W, 2, 4, 4, 2, drop_p=0.1, drop_seed=3)
    kvb = b(8, 2 * W)
    with pytest.raises(ValueError):
        ops.attention_fwd_ex(q, W, kvb, kvb[:, W:], 2 * W, 2, 4, 4, 2)
    with pytest.raises(ValueError):
        ops.attention_fwd_ex(b(8, W), W, kv, kv[:, W:], 2 * W, 2, 4, 4, 2)
    with pytest.raises(NotImplementedError):          # the general form has no fp16 entry point: refused, not run in another type
        ops.attention_fwd_ex(q, W, kv, kv[:, W:], 2 * W, 2, 4, 4, 2)
    with pytest.raises(ValueError):
        ops.attention_fwd(h(8, 3 * W), 2, 4, 2, False, out=b(8, W))
    with pytest.raises(ValueError):
        ops.attention_fwd(h(8, 3 * W), 2, 4, 2, True)
    with pytest.raises(ValueError):
        ops.linear_fwd(h(8, W), b(16, W))
    with pytest.raises(ValueError):
        ops.linear_fwd(b(8, W), h(16, W))
    with pytest.raises(ValueError):
        ops.linear_fwd(h(8, W), h(16, W), out=h(8, 16), epilogue=ops.EPI_BIAS_ACT, C2=b(8, 16))


def test_linear_fwd_passes_the_type_of_its_operand(monkeypatch):
    """bf16 callers get the descriptor they always got (dtype 0, bf16 output); an fp16 x gives UNIIR_DT_F16 and fp16 outputs"""
    from uniir_amd import ops
    seen = []
    monkeypatch.setattr(ops, "gemm", lambda A, B, out, *a, **k: (seen.append((a, k)), out)[1])
    for dt, code in ((torch.bfloat16, ops.DT_BF16), (torch.float16, ops.DT_F16)):
        x, w = torch.zeros(8, 64, dtype=dt), torch.zeros(16, 64, dtype=dt)
        assert ops.linear_fwd(x, w).dtype == dt
        assert ops.linear_fwd(x, w, epilogue=ops.EPI_RESID_F32).dtype == torch.float32
        assert ops.linear_fwd(x, w, out=torch.zeros(8, 16), epilogue=ops.EPI_F32).dtype == torch.float32
        assert [k["dtype"] for _, k in seen[-3:]] == [code] * 3
        assert seen[-3][0] == (8, 16, 64, 64, 64, 16)


def test_the_fp16_tower_forward_keeps_nothing_for_a_backward():
    from uniir_amd import resblocks
    x = torch.zeros(4, 64)
    with pytest.raises(RuntimeError, match="save=True"):
        resblocks.tower_fwd(None, None, 1, x, 1, 4, 64, 1, False, True, dtype16=torch.float16)
    with pytest.raises(ValueError):
        resblocks.tower_fwd(None, None, 1, x, 1, 4, 64, 1, False, False, dtype16=torch.float32)


# (entry point, its bf16 twin, a well-formed call as a dict, the changes that each must be refused with the twin's code)
_LN = dict(x=0x10000, x_stride=64, gamma=0x20000, beta=0x30000, y16=0x40000, y32=0x50000, rows=4, width=64, eps=1e-5, stream=None)
_PF = dict(images=0x10000, patches=0x20000, n=2, res=32, patch=16, kpad=768, stream=None)
_VA = dict(po=0x10000, cls=0x20000, pos=0x30000, x=0x40000, n=2, tokens=5, width=64, stream=None)
_GLUE = [
    ("uniir_layernorm_fwd_f16", "uniir_layernorm_fwd", _LN,
     [dict(x=None), dict(gamma=None), dict(beta=None), dict(y16=None, y32=None), dict(rows=-1), dict(rows=0), dict(width=66),
      dict(width=0), dict(width=2052), dict(x_stride=66), dict(rows=0, width=66)]),
    ("uniir_patchify_f16", "uniir_patchify", _PF,
     [dict(images=None), dict(patches=None), dict(n=-1), dict(n=0), dict(patch=0), dict(res=40), dict(kpad=772), dict(kpad=760),
      dict(n=0, kpad=760)]),
    ("uniir_vit_assemble_f16", "uniir_vit_assemble", _VA,
     [dict(po=None), dict(cls=None), dict(pos=None), dict(x=None), dict(n=-1), dict(n=0), dict(width=66), dict(tokens=1),
      dict(n=0, tokens=1)]),
]


@pytest.mark.parametrize("fn,twin,ok,changes", _GLUE, ids=[g[0] for g in _GLUE])
def test_the_fp16_glue_entry_points_keep_the_checks_of_their_bf16_twins(fn, twin, ok, changes):
    from uniir_amd import _lib
    lib = _lib.load()
    assert _lib.SIGNATURES[fn] == _lib.SIGNATURES[twin]
    count = "rows" if "rows" in ok else "n"          # the argument whose 0 makes a call empty
    codes = set()
    for ch in changes:
        call = {**ok, **ch}
        got, want = getattr(lib, fn)(*call.values()), getattr(lib, twin)(*call.values())
        assert got == want, (fn, ch, got, want)
        assert got < 0 or call[count] == 0, (fn, ch, got)          # 0 only for an empty call: nothing here may reach a launch
        codes.add(got)
    assert codes == {0, -1, -2}          # UNIIR_OK for an empty call, UNIIR_EINVAL, UNIIR_ESHAPE: every branch was reached


# ---- the padded copies and the two "the masters moved" events: the exact ops.call sequence of every event ----------------------------
PAD = ("conv.weight", 8, 27, 64)          # an 8 x 27 tensor, rows padded to 64


@pytest.fixture
def padded_store(monkeypatch):
    """a CPU store with gradients and one padded tensor registered, its device calls recorded"""
    from uniir_amd import flat_store
    calls = []
    monkeypatch.setattr(flat_store.ops, "call", lambda name, *a: calls.append((name,) + a))
    st = flat_store.FlatStore([("conv.weight", (8, 3, 3, 3))] + SHAPES, "cpu")
    st.add_padded(*PAD)
    st.calls = calls
    return st


def _taken(st):
    """the calls recorded since the last look, as (name, what was written, the scalars); the source is checked here"""
    out = []
    for name, src, dst, *rest in st.calls:
        whole = name in ("uniir_cast_f32_to_bf16", "uniir_cast_f32_to_f16")
        want = st.p32 if whole else st.p("conv.weight")
        assert src.data_ptr() == want.data_ptr() and src.dtype == torch.float32 and (src is st.p32) == whole
        out.append((name, dst, tuple(rest)))
    del st.calls[:]
    return out


def test_every_event_makes_exactly_its_calls(padded_store):
    st = padded_store
    assert st.calls == [] and st.half_bytes() == 0          # construction and registration launch nothing, allocate no fp16
    b16 = st.padded16("conv.weight")
    assert b16.dtype == torch.bfloat16 and tuple(b16.shape) == (8, 64)
    g = st.padded_grad("conv.weight")
    assert g.dtype == torch.float32 and tuple(g.shape) == (8, 64) and g.data_ptr() != st.g32.data_ptr()
    pad16 = ("uniir_cast_pad_rows", b16, (8, 27, 64))
    st.refresh_shadow()
    assert _taken(st) == [("uniir_cast_f32_to_bf16", st.w16_buf, (st.total,)), pad16]
    st.kernel_wrote()          # the kernel cast the flat shadow itself: only the padded copy is left to do
    assert _taken(st) == [pad16]
    assert st.half_bytes() == 0 and st.h16_buf is None          # neither event touches fp16
    h = st.half_shadow()          # the first one: allocates, one cast and one fp16 pad
    h16 = st.padded16h("conv.weight")
    assert h is st.h16_buf and h16.dtype == torch.float16 and tuple(h16.shape) == (8, 64) and st.half_bytes() == 2 * (st.total + 8 * 64)
    padh = ("uniir_cast_pad_rows_f16", h16, (8, 27, 64))
    assert _taken(st) == [("uniir_cast_f32_to_f16", h, (st.total,)), padh]
    st.half_shadow()          # a second one: nothing
    st.w16h("a.weight")
    assert _taken(st) == []
    for event, calls in ((st.refresh_shadow, [("uniir_cast_f32_to_bf16", st.w16_buf, (st.total,)), pad16]), (st.kernel_wrote, [pad16])):
        event()
        assert _taken(st) == calls and st.half_stale is True          # fp16 is marked, not cast
        assert st.half_shadow() is h and st.padded16h("conv.weight") is h16          # refilled in place: raw pointers stay valid
        assert _taken(st) == [("uniir_cast_f32_to_f16", h, (st.total,)), padh]
        st.half_shadow()
        assert _taken(st) == []
    assert st.padded16("conv.weight") is b16 and st.padded_grad("conv.weight") is g


def test_a_store_without_padded_tensors_makes_no_pad_call_and_one_without_gradients_keeps_no_scratch(store, monkeypatch):
    from uniir_amd import flat_store
    store.refresh_shadow()
    store.kernel_wrote()
    store.half_shadow()
    store.kernel_wrote()
    store.half_shadow()
    assert [c[0] for c in store.calls] == ["uniir_cast_f32_to_bf16", "uniir_cast_f32_to_f16", "uniir_cast_f32_to_f16"]
    assert store.half_bytes() == 2 * store.total
    mom = flat_store.FlatStore([("conv.weight", (8, 3, 3, 3))], "cpu", with_grad=False)          # the BLIP momentum store's kind
    mom.add_padded(*PAD)
    assert mom.padded_grad("conv.weight") is None and mom.padded16("conv.weight").shape == (8, 64)
    with pytest.raises(ValueError):
        mom.add_padded("conv.weight", 8, 28, 64)          # not the tensor's element count
    with pytest.raises(ValueError):
        mom.add_padded("conv.weight", 8, 27, 16)          # a leading dimension below the row length
    assert flat_store.patch_kpad(16) == 768 and flat_store.patch_kpad(14) == 640 and flat_store.patch_kpad(3) == 64


def test_sync_refreshes_exactly_when_a_watched_parameter_was_written_on_the_torch_side(monkeypatch):
    from uniir_amd import flat_store
    calls = []
    monkeypatch.setattr(flat_store.ops, "call", lambda name, *a: calls.append(name))
    mod = torch.nn.Module()
    mod.conv = torch.nn.Parameter(torch.randn(8, 3, 3, 3))
    mod.w = torch.nn.Parameter(torch.randn(6, 10))
    mod.temp = torch.nn.Parameter(torch.tensor(0.07))
    st = flat_store.FlatStore.adopt(list(mod.named_parameters()), "cpu", unversioned=("temp",))
    st.add_padded("conv", 8, 27, 64)
    refresh = ["uniir_cast_f32_to_bf16", "uniir_cast_pad_rows"]

    def synced():
        del calls[:]
        st.sync()
        return list(calls)

    assert synced() == refresh          # nothing was cast yet
    assert synced() == [] and synced() == []          # no version moved
    st.kernel_wrote()          # a kernel's writes move no version
    assert synced() == []
    with torch.no_grad():
        mod.w[2, :3] += 1.0
    assert synced() == refresh and synced() == []          # an in-place edit of any adopted parameter: one refresh
    with torch.no_grad():
        mod.conv.mul_(2.0)
        mod.w.mul_(2.0)
    assert synced() == refresh and synced() == []          # however many moved
    with torch.no_grad():
        mod.temp.clamp_(0.001, 0.5)
    assert synced() == []          # an unversioned one: none
    mod.load_state_dict({k: v.detach().clone() + 1 for k, v in mod.state_dict().items()})
    assert st.holds(mod.named_parameters()) and synced() == refresh and synced() == []          # load_state_dict: one
    assert float(st.p("temp")) == float(mod.temp.detach()) and st.half_bytes() == 0
    st.half_shadow()
    with torch.no_grad():
        mod.w[0, 0] = 3.0
    st.sync()
    assert st.half_stale is True          # ... and the fp16 copies follow at their next use
