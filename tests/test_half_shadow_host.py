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
    store.mark_half_stale()
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
    store.mark_half_stale()          # a writer that goes past the class (fused AdamW, EMA)
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
