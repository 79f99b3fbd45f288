"""Host side of the fp16 general attention form and of the BLIP fp16 embedding forward (no device):
  the binding and the wrappers know uniir_attn_general_fwd_f16 and uniir_onequery_fwd_f16, and neither name starts with
  uniir_attention_ (tests/test_attention_refusals_host.py pins that family at 17);
  every call the two entry points refuse returns its documented code, in the documented order, and writes nothing (a refused call
  returns before any HIP call) -- the pattern of tests/test_onequery_ref.py;
  the wrappers refuse operands that are not all fp16 before any launch, and ops.attention_fwd_ex keeps refusing fp16;
  bert_forward's fp16 forward keeps nothing for a backward and takes no dropout, an unknown precision raises, and the embedder's
  _tower_precision flips a BLIP module only when both use_fp16 and embed_fp16 are set -- and puts it back."""
import ctypes as C
import types

import pytest
import torch

ERR = {"OK": 0, "EINVAL": -1, "ESHAPE": -2, "EALIGN": -3}
GENERAL = ("q", "q_ld", "k", "v", "kv_ld", "out", "out_ld", "lse", "q_row_off", "kv_packed", "key_len", "batch", "tq", "tk", "heads")
ONEQ = ("q", "q_ld", "k", "v", "kv_ld", "out", "out_ld", "lse", "key_len", "kv_row_off", "batch", "tk", "heads")
NAMES = {"uniir_attn_general_fwd_f16": GENERAL, "uniir_onequery_fwd_f16": ONEQ}
POINTERS = {"q", "k", "v", "out", "lse", "q_row_off", "key_len", "kv_row_off"}
OPTIONAL = {"q_row_off", "key_len", "kv_row_off"}
LDS = {"q_ld", "kv_ld", "out_ld"}
ALIGNED = {"q", "k", "v", "out"}          # the pointers whose alignment is tested


def test_the_binding_and_the_wrappers_know_the_entry_points():
    from uniir_amd import _lib, ops
    lib = _lib.load()
    for name, nargs in (("uniir_attn_general_fwd_f16", 16), ("uniir_onequery_fwd_f16", 14)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and getattr(lib, name).argtypes is not None
        assert not name.startswith("uniir_attention_")
        assert len(NAMES[name]) + 1 == nargs          # + the stream
    assert callable(ops.attention_fwd_ex_f16) and callable(ops.onequery_fwd_f16)


def _refusal_table():
    """(entry point, what changes, {argument: value}, code); pointer values are byte offsets into the test's buffer, "keep" a valid
    pointer for an optional argument that the good call leaves NULL"""
    rows = []
    for fn, names in NAMES.items():
        for p in names:
            if p in POINTERS and p not in OPTIONAL:
                rows.append((fn, f"{p} NULL", {p: None}, "EINVAL"))
            if p in ALIGNED:
                rows.append((fn, f"{p} + 8 bytes", {p: "+8"}, "EALIGN"))
            if p in LDS:
                rows.append((fn, f"{p} + 4", {p: "+4"}, "EALIGN"))
        rows += [(fn, "heads 0", {"heads": 0}, "EINVAL"), (fn, "heads -1", {"heads": -1}, "EINVAL"),
                 (fn, "batch -1", {"batch": -1}, "EINVAL"),
                 (fn, "tk 0", {"tk": 0}, "ESHAPE"), (fn, "tk 1025", {"tk": 1025}, "ESHAPE"), (fn, "tk -3", {"tk": -3}, "ESHAPE"),
                 (fn, "tk 1025 and a bad kv_ld", {"tk": 1025, "kv_ld": "+4"}, "ESHAPE"),
                 (fn, "a bad kv_ld and q + 8 bytes", {"kv_ld": "+4", "q": "+8"}, "EALIGN"),
                 (fn, "batch 0", {"batch": 0}, "OK"),
                 (fn, "batch 0, tk 0, q + 8 bytes", {"batch": 0, "tk": 0, "q": "+8"}, "OK"),
                 (fn, "batch 0, q NULL", {"batch": 0, "q": None}, "EINVAL")]
    g = "uniir_attn_general_fwd_f16"
    rows += [(g, "tq 0", {"tq": 0}, "ESHAPE"), (g, "tq 1025", {"tq": 1025}, "ESHAPE"), (g, "tq -3", {"tq": -3}, "ESHAPE"),
             # check 2: every misuse of kv_packed, each before batch == 0 and before the sizes
             (g, "kv_packed without q_row_off", {"kv_packed": 1, "tq": 16}, "EINVAL"),
             (g, "kv_packed with key_len", {"kv_packed": 1, "tq": 16, "q_row_off": "keep", "key_len": "keep"}, "EINVAL"),
             (g, "kv_packed with tq != tk", {"kv_packed": 1, "tq": 8, "q_row_off": "keep"}, "EINVAL"),
             (g, "kv_packed with tq != tk, batch 0", {"kv_packed": 1, "tq": 8, "q_row_off": "keep", "batch": 0}, "EINVAL"),
             (g, "kv_packed without q_row_off, tq = tk = 0", {"kv_packed": 1, "tq": 0, "tk": 0}, "EINVAL"),
             (g, "kv_packed with tq 513", {"kv_packed": 1, "tq": 513, "tk": 513, "q_row_off": "keep"}, "ESHAPE"),
             (g, "kv_packed with tq 513 and a bad q_ld", {"kv_packed": 1, "tq": 513, "tk": 513, "q_row_off": "keep", "q_ld": "+4"}, "ESHAPE"),
             (g, "kv_packed, batch 0, tq 513", {"kv_packed": 1, "tq": 513, "tk": 513, "q_row_off": "keep", "batch": 0}, "OK"),
             (g, "batch 0, tq 1025, k + 8 bytes", {"batch": 0, "tq": 1025, "k": "+8"}, "OK")]
    o = "uniir_onequery_fwd_f16"
    rows += [(o, "both key forms", {"key_len": "keep", "kv_row_off": "keep"}, "EINVAL"),
             (o, "both key forms, tk 0", {"key_len": "keep", "kv_row_off": "keep", "tk": 0}, "EINVAL"),          # pins the order
             (o, "both key forms, batch 0", {"key_len": "keep", "kv_row_off": "keep", "batch": 0}, "EINVAL")]
    return rows


REFUSALS = _refusal_table()


@pytest.mark.parametrize("fn", sorted(NAMES))
def test_refused_calls_return_their_code_and_write_nothing(fn):
    from uniir_amd import _lib
    lib = _lib.load()
    names = NAMES[fn]
    assert len(_lib.SIGNATURES[fn][1]) == len(names) + 1          # + the stream
    n = 1 << 16
    raw = C.create_string_buffer(n + 256)
    base = (C.addressof(raw) + 255) & ~255
    pattern = bytes((7 * i + 3) & 255 for i in range(n))
    W = 128
    good = dict(q_ld=W, kv_ld=2 * W, out_ld=W, kv_packed=0, batch=1, tq=4, tk=16, heads=2)
    slot = {p: 4096 * (i + 1) for i, p in enumerate(sorted(POINTERS))}
    for p in POINTERS:
        good[p] = None if p in OPTIONAL else slot[p]
    rows = [r for r in REFUSALS if r[0] == fn]
    assert {r[3] for r in rows} == set(ERR)          # every one of the four codes is reached
    for r in rows:          # no row may reach a launch: checked for ALL rows before the first call
        assert r[3] != "OK" or r[2].get("batch") == 0, r
    wrong = []
    for _, what, change, code in rows:
        a = dict(good)
        for k, val in change.items():
            if val == "keep":
                a[k] = slot[k]
            elif isinstance(val, str):
                a[k] = good[k] + int(val)
            else:
                a[k] = val
        vals = [(None if a[p] is None else base + a[p]) if p in POINTERS else a[p] for p in names]
        C.memmove(base, pattern, n)
        rc = getattr(lib, fn)(*vals, None)
        if rc != ERR[code]:
            wrong.append((what, code, rc))
        assert C.string_at(base, n) == pattern, what
    assert not wrong, wrong


def test_the_wrappers_take_fp16_operands_only():
    from uniir_amd import ops
    W = 128
    h = lambda *s: torch.zeros(*s, dtype=torch.float16)          # noqa: E731
    b = lambda *s: torch.zeros(*s, dtype=torch.bfloat16)         # noqa: E731
    q, kv, qb, kvb = h(8, W), h(8, 2 * W), b(8, W), b(8, 2 * W)
    for qq, kk, vv in ((qb, kvb, kvb[:, W:]), (qb, kv, kv[:, W:]), (q, kvb, kvb[:, W:]), (q, kv, kvb[:, W:]), (q, kvb, kv[:, W:])):
        with pytest.raises(ValueError):
            ops.attention_fwd_ex_f16(qq, W, kk, vv, 2 * W, 2, 4, 4, 2)
        with pytest.raises(ValueError):
            ops.onequery_fwd_f16(qq, W, kk, vv, 2 * W, 2, 4, 2)
    with pytest.raises(ValueError):
        ops.attention_fwd_ex_f16(torch.zeros(8, W), W, kv, kv[:, W:], 2 * W, 2, 4, 4, 2)          # fp32 is no fp16 either
    with pytest.raises(NotImplementedError):          # the bf16 wrapper keeps refusing fp16: the fp16 form has wrappers of its own
        ops.attention_fwd_ex(q, W, kv, kv[:, W:], 2 * W, 2, 4, 4, 2)
    with pytest.raises(RuntimeError, match="device tensors"):          # all fp16: past the type check, and no CPU path behind it
        ops.attention_fwd_ex_f16(q, W, kv, kv[:, W:], 2 * W, 2, 4, 4, 2)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.onequery_fwd_f16(q, W, kv, kv[:, W:], 2 * W, 2, 4, 2)


# ----------------------------------------------------------------------------------------------------------------- model host logic
MED_TINY = dict(hidden_size=128, intermediate_size=256, num_attention_heads=2, num_hidden_layers=1, vocab_size=64,
                max_position_embeddings=32)
VIT_TINY = dict(img_size=32, patch_size=16, embed_dim=128, depth=1, num_heads=2, drop_path_rate=0.0)


def test_the_fp16_bert_forward_keeps_nothing_for_a_backward_and_takes_no_dropout():
    from uniir_amd import blip_model as bm, ops
    cfg = {**bm.MED_DEFAULT, **MED_TINY}
    ids, kl = torch.zeros(2, 4, dtype=torch.int32), torch.full((2,), 4, dtype=torch.int32)
    img = torch.zeros(2 * 5, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="save=True"):
        bm.bert_forward(None, "text_encoder.", cfg, ids, kl, img, 5, True, dtype16=torch.float16)
    with pytest.raises(RuntimeError, match="dropout"):
        bm.bert_forward(None, "text_encoder.", cfg, ids, kl, img, 5, False, drop=ops.DropSeeds(), dtype16=torch.float16)
    with pytest.raises(ValueError):          # bf16 image tokens with an fp16 forward
        bm.bert_forward(None, "text_encoder.", cfg, ids, kl, img.to(torch.bfloat16), 5, False, dtype16=torch.float16)
    with pytest.raises(ValueError):
        bm.bert_forward(None, "text_encoder.", cfg, ids, kl, img, 5, False, dtype16=torch.float32)


@pytest.mark.parametrize("cls", ["BLIPFeatureFusion", "BLIPScoreFusion"])
def test_precision_is_bf16_by_default_and_anything_but_bf16_or_fp16_raises(cls, monkeypatch):
    from uniir_amd import blip_model as bm
    monkeypatch.delenv("UNIIR_BLIP_EMBED_FP16", raising=False)
    make = lambda: getattr(bm, cls)(med_config=MED_TINY, vit_config=VIT_TINY, embed_dim=128, queue_size=16, momentum=0.9,      # noqa: E731
                                    config=types.SimpleNamespace(tokenizer_max_length=4), seed=0)
    model = make().eval()
    assert model.precision == "bf16" and model.embed_fp16 is False
    monkeypatch.setenv("UNIIR_BLIP_EMBED_FP16", "1")
    assert make().embed_fp16 is True and make().precision == "bf16"          # the switch opts in; it does not change the default
    txt = types.SimpleNamespace(input_ids=torch.zeros(2, 4, dtype=torch.int64), attention_mask=torch.ones(2, 4, dtype=torch.int64))
    img = torch.zeros(2, 3, 32, 32)
    for bad in ("fp32", "FP16", None):
        model.precision = bad
        with pytest.raises(RuntimeError, match="unknown precision"):
            model.encode_multimodal_input(txt, img)
    model.precision = "fp16"
    model.train()
    with pytest.raises(RuntimeError, match="eval"):
        model.encode_multimodal_input(txt, img)
    model.eval()
    with pytest.raises(RuntimeError, match="online"):
        model.encode_multimodal_input(txt, img, use_momentum=True)


def _embedder():
    import os
    import sys
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "uniir_amd", "src")
    for p in (src, os.path.join(src, "common")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import mbeir_embedder
    return mbeir_embedder


class _Blip:
    def __init__(self, embed_fp16, precision="bf16"):
        self.embed_fp16, self.precision = embed_fp16, precision


@pytest.mark.parametrize("wrap", [False, True], ids=["bare", "module"])
def test_tower_precision_flips_a_blip_model_only_when_it_opted_in_and_restores_it(wrap):
    E = _embedder()
    seen = []
    for use_fp16 in (False, True):
        for embed_fp16 in (False, True):
            blip = _Blip(embed_fp16)
            model = types.SimpleNamespace(module=blip) if wrap else blip
            with E._tower_precision(model, use_fp16):
                seen.append(blip.precision)
            assert blip.precision == "bf16"
            with pytest.raises(KeyError):          # restored when the body raises, too
                with E._tower_precision(model, use_fp16):
                    assert blip.precision == seen[-1]
                    raise KeyError("body")
            assert blip.precision == "bf16"
    assert seen == ["bf16", "bf16", "bf16", "fp16"]
    # a model that was set to fp16 by hand stays there, inside and afterwards
    blip = _Blip(True, "fp16")
    with E._tower_precision(types.SimpleNamespace(module=blip) if wrap else blip, True):
        assert blip.precision == "fp16"
    assert blip.precision == "fp16"


@pytest.mark.parametrize("wrap", [False, True], ids=["bare", "module"])
def test_tower_precision_leaves_the_handling_of_a_clip_model_as_it_is(wrap):
    E = _embedder()
    for use_fp16, inside in ((False, "bf16"), (True, "fp16")):
        clip = types.SimpleNamespace(precision="bf16")
        inner = types.SimpleNamespace(clip_model=clip)          # no embed_fp16: CLIP needs no opt-in
        model = types.SimpleNamespace(module=inner) if wrap else inner
        with E._tower_precision(model, use_fp16):
            assert clip.precision == inside
        assert clip.precision == "bf16"
        with pytest.raises(KeyError):
            with E._tower_precision(model, use_fp16):
                raise KeyError("body")
        assert clip.precision == "bf16"
    plain = types.SimpleNamespace()          # neither: nothing to flip, nothing raised
    with E._tower_precision(plain, True):
        pass


# ------------------------------------------------------------------------------------------- the launch sequence of bert_forward
def _recorded_bert_forward(monkeypatch, dtype16, pool_last):
    """bert_forward (one layer, cross-attention, pooler, dense rows) on a CPU store with every op recorded instead of launched ->
    the list of what it called"""
    from uniir_amd import blip_model as bm, flat_store, ops
    cfg = {**bm.MED_DEFAULT, **MED_TINY}
    W, E, M, Lq, Ti, H = cfg["hidden_size"], 192, 2, 4, 5, cfg["num_attention_heads"]
    st = flat_store.FlatStore([("text_encoder." + n, s) for n, s in bm.bert_param_shapes(cfg, E)], "cpu")
    seen = []
    f32 = (ops.EPI_RESID_F32, ops.EPI_F32)

    def call(name, *a):
        seen.append(("call", name))

    def linear_fwd(x, w, bias=None, *, out=None, epilogue=ops.EPI_BF16, resid=None, C2=None, act=ops.ACT_QUICKGELU, row_scale=None):
        seen.append(("linear", x.dtype, w.dtype, tuple(w.shape), epilogue, None if C2 is None else C2.dtype, resid is not None))
        return out if out is not None else torch.empty(x.shape[0], w.shape[0], dtype=torch.float32 if epilogue in f32 else x.dtype)

    def layernorm_fwd(x, gamma, beta, eps=1e-5, *, out_bf16=None, out_f32=None, rows=None, width=None, **kw):
        seen.append(("ln", out_bf16.dtype, out_f32.dtype, rows, width, sorted(kw)))

    def attn(tag, dt):
        def f(q, q_ld, k, v, kv_ld, batch, tq, tk, heads, **kw):
            seen.append((tag, q.dtype, k.dtype, v.dtype, q_ld, kv_ld, batch, tq, tk, heads, sorted(kw)))
            return torch.empty(batch * tq, heads * 64, dtype=dt), torch.empty(batch, heads, tq)
        return f

    def oneq(tag, dt):
        def f(q, q_ld, k, v, kv_ld, batch, tk, heads, **kw):
            seen.append((tag, q.dtype, k.dtype, v.dtype, q_ld, kv_ld, batch, tk, heads, sorted(kw)))
            return torch.empty(batch, heads * 64, dtype=dt), torch.empty(batch, heads)
        return f

    for name, fn in (("call", call), ("linear_fwd", linear_fwd), ("layernorm_fwd", layernorm_fwd),
                     ("attention_fwd_ex", attn("attention_fwd_ex", torch.bfloat16)), ("attention_fwd_ex_f16", attn("attention_fwd_ex_f16", torch.float16)),
                     ("onequery_fwd", oneq("onequery_fwd", torch.bfloat16)), ("onequery_fwd_f16", oneq("onequery_fwd_f16", torch.float16))):
        monkeypatch.setattr(ops, name, fn)
    ids, kl = torch.zeros(M, Lq, dtype=torch.int32), torch.full((M,), Lq, dtype=torch.int32)
    img = torch.zeros(M * Ti, E, dtype=dtype16)
    kw = {} if dtype16 == torch.bfloat16 else dict(dtype16=dtype16)          # the bf16 caller: the call as it always was written
    pooled, stash = bm.bert_forward(st, "text_encoder.", cfg, ids, kl, img, Ti, False, pool_last=pool_last, **kw)
    assert pooled.dtype == torch.float32 and pooled.shape == (M, W) and stash is None
    return seen, (W, E, M, Lq, Ti, H, cfg["intermediate_size"])


@pytest.mark.parametrize("pool_last", [False, True], ids=["full", "pool_last"])
def test_a_bf16_caller_makes_the_calls_it_always_made_and_fp16_is_the_same_sequence_in_fp16(monkeypatch, pool_last):
    from uniir_amd import ops
    B, F = torch.bfloat16, torch.float32
    got, (W, E, M, Lq, Ti, H, I) = _recorded_bert_forward(monkeypatch, B, pool_last)
    R = M * Lq
    Rl = M if pool_last else R          # the rows behind the q | k | v projection of the (only, hence last) layer
    drop = ["drop_p", "drop_seed"]
    if pool_last:
        self_attn = ("onequery_fwd", B, B, B, Lq * 3 * W, 3 * W, M, Lq, H, sorted(drop + ["drop_q", "drop_tq", "key_len"]))
        cross_attn = ("onequery_fwd", B, B, B, W, 2 * W, M, Ti, H, sorted(drop + ["drop_q", "drop_tq"]))
    else:
        self_attn = ("attention_fwd_ex", B, B, B, 3 * W, 3 * W, M, Lq, Lq, H, sorted(drop + ["key_len"]))
        cross_attn = ("attention_fwd_ex", B, B, B, W, 2 * W, M, Lq, Ti, H, drop)
    want = [("call", "uniir_text_embed"), ("ln", B, F, R, W, []),
            ("linear", B, B, (3 * W, W), ops.EPI_BF16, None, False), self_attn]
    if pool_last:
        want.append(("call", "uniir_gather_rows"))
    want += [("linear", B, B, (W, W), ops.EPI_RESID_F32, None, True), ("ln", B, F, Rl, W, []),
             ("linear", B, B, (W, W), ops.EPI_BF16, None, False), ("linear", B, B, (2 * W, E), ops.EPI_BF16, None, False), cross_attn,
             ("linear", B, B, (W, W), ops.EPI_RESID_F32, None, True), ("ln", B, F, Rl, W, []),
             ("linear", B, B, (I, W), ops.EPI_BIAS_ACT, B, False), ("linear", B, B, (W, I), ops.EPI_RESID_F32, None, True),
             ("ln", B, F, Rl, W, [])]
    if not pool_last:
        want.append(("call", "uniir_gather_rows"))
    want += [("call", "uniir_cast_f32_to_bf16"), ("linear", B, B, (W, W), ops.EPI_RESID_F32, None, False), ("call", "uniir_tanh_fwd")]
    assert got == want
    # fp16: one cast of the whole store into the fp16 shadow, then the same sequence with fp16 in place of bf16, the fp16 attention
    # wrappers without the dropout arguments and the fp16 cast
    half, _ = _recorded_bert_forward(monkeypatch, torch.float16, pool_last)
    H16 = torch.float16

    def as_fp16(c):
        c = tuple(H16 if x is B else x for x in c)
        if c[0] in ("attention_fwd_ex", "onequery_fwd"):
            c = (c[0] + "_f16",) + c[1:-1] + ([k for k in c[-1] if not k.startswith("drop_")],)
        return ("call", "uniir_cast_f32_to_f16") if c == ("call", "uniir_cast_f32_to_bf16") else c

    shadow = [("call", "uniir_cast_f32_to_f16")]
    assert half.count(shadow[0]) == 2          # the shadow once (not once per weight), and the class rows
    first = half.index(shadow[0])
    assert half[:first] + half[first + 1:] == [as_fp16(c) for c in want]
