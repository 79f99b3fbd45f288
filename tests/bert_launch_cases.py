"""The launch sequence of blip_model.bert_forward / bert_backward as data (tests/test_blip_bert_launches_host.py and
tests/golden/make_golden_bert_launches.py): every ops function the MED BERT uses is replaced by a recorder that appends one entry and
returns tensors of the right shape and dtype, on a CPU FlatStore -- no GPU, no library.

An entry is [op, positional arguments, keyword arguments, what it returned].  A tensor is the string
    <dtype>[shape](stride)+<storage offset>@<buffer>
where <buffer> is p32 / g32 / w16 / h16 for a view of the flat store (the offset then says which parameter, gradient slice or span)
and #n for any other buffer, numbered in the order the trace first met them (the same n = the same memory: which activation went where;
the column views of qkv / ckv / dqkv differ in the offset).  Scalars stand verbatim (the dropout seeds after torch.manual_seed, drop_tq /
drop_q / kv_packed / rows).  The trace ends with the log lines of a class-row pass and the shape of the returned dimg."""
import contextlib
import hashlib
import itertools
import json

import torch

W, HEADS, I, ENC, M, L, TI = 128, 2, 256, 192, 3, 5, 4
KEY_LEN = (5, 2, 3)          # one caption full, the others ragged: packing is real
SEED = 1234
RECORDED = ("call", "linear_fwd", "layernorm_fwd", "layernorm_bwd", "linear_dgrad", "linear_wgrad", "gemm", "attention_fwd_ex",
            "attention_fwd_ex_f16", "onequery_fwd", "onequery_fwd_f16", "attention_bwd_ex", "onequery_bwd", "dropout_f32", "dropout_bf16_")


def _cases():
    out = []
    for model, pack, pool_last, drop, layers in itertools.product(("FF", "SF"), (True, False), (True, False), (True, False), (1, 2)):
        out.append(dict(dtype="bf16", model=model, pack=pack, pool_last=pool_last, drop=drop, layers=layers))
    for model, pack, pool_last, layers in itertools.product(("FF", "SF"), (True, False), (True, False), (1, 2)):
        out.append(dict(dtype="fp16", model=model, pack=pack, pool_last=pool_last, drop=False, layers=layers))
    return out


CASES = _cases()


def name_of(c):
    return "-".join([c["dtype"], c["model"], "packed" if c["pack"] else "dense", "pool_last" if c["pool_last"] else "full",
                     "drop" if c["drop"] else "nodrop", f"{c['layers']}L"])


NAMES = [name_of(c) for c in CASES]
_DT = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16", torch.int32: "i32", torch.int64: "i64"}


class Recorder:
    def __init__(self, st):
        self.st, self.entries, self.seen, self.keep = st, [], {}, []

    def tensor(self, t):
        ptr = t.untyped_storage().data_ptr()
        st = self.st
        bufs = {"p32": st.p32, "g32": st.g32, "w16": st.w16_buf, "h16": st.h16_buf}
        tag = next((n for n, b in bufs.items() if b is not None and b.untyped_storage().data_ptr() == ptr), None)
        if tag is None:
            if ptr not in self.seen:
                self.seen[ptr] = f"#{len(self.seen)}"
                self.keep.append(t)          # alive to the end of the trace: an address is never met twice
            tag = self.seen[ptr]
        return f"{_DT[t.dtype]}{list(t.shape)}({','.join(map(str, t.stride()))})+{t.storage_offset()}@{tag}"

    def enc(self, v):
        if isinstance(v, torch.Tensor):
            return self.tensor(v)
        if isinstance(v, (tuple, list)):
            return [self.enc(x) for x in v]
        if isinstance(v, torch.dtype):
            return _DT[v]
        assert v is None or isinstance(v, (bool, int, float, str)), type(v)
        return v

    def wrap(self, name, result):
        def f(*a, **kw):
            entry = [name, self.enc(a), {k: self.enc(v) for k, v in sorted(kw.items())}, None]
            self.entries.append(entry)
            out = result(*a, **kw)
            entry[3] = self.enc(out)
            return out
        return f


def _fakes():
    """op -> what it returns: the shapes and dtypes of uniir_amd.ops"""
    from uniir_amd import ops
    f32_out = (ops.EPI_RESID_F32, ops.EPI_F32)

    def nothing(*a, **kw):
        return None

    def linear_fwd(x, w, bias=None, *, out=None, epilogue=ops.EPI_BF16, resid=None, C2=None, act=ops.ACT_QUICKGELU, row_scale=None):
        return out if out is not None else torch.empty(x.shape[0], w.shape[0], dtype=torch.float32 if epilogue in f32_out else x.dtype)

    def layernorm_fwd(x, gamma, beta, eps=1e-5, *, out_bf16=None, out_f32=None, rows=None, width=None, x_stride=None,
                      dtype16=torch.bfloat16):
        if out_bf16 is None and out_f32 is None:
            out_bf16 = torch.empty(rows, width, dtype=dtype16)
        return out_bf16 if out_bf16 is not None else out_f32

    def layernorm_bwd(x, gamma, dy, dgamma, dbeta, eps=1e-5, *, dres=None, dx=None, dx_bf16=None, rows=None, width=None, x_stride=None,
                      dx_stride=None, dx_colsum=None, branch_scale=None):
        return dx if dx is not None else torch.empty(rows, width, dtype=torch.float32)

    def linear_dgrad(dy, w, *, out=None, aux=None, act=ops.ACT_QUICKGELU, act_out=None, colsum=None):
        return out if out is not None else torch.empty(dy.shape[0], w.shape[1], dtype=torch.bfloat16)

    def gemm(A, B, C_out, *a, **kw):
        return C_out

    def attn(dt):
        def f(q, q_ld, k, v, kv_ld, batch, tq, tk, heads, *, rows=None, **kw):
            return torch.empty(batch * tq if rows is None else rows, heads * 64, dtype=dt), torch.empty(batch, heads, tq)
        return f

    def oneq(dt):
        def f(q, q_ld, k, v, kv_ld, batch, tk, heads, **kw):
            return torch.empty(batch, heads * 64, dtype=dt), torch.empty(batch, heads)
        return f

    return dict(call=nothing, linear_fwd=linear_fwd, layernorm_fwd=layernorm_fwd, layernorm_bwd=layernorm_bwd, linear_dgrad=linear_dgrad,
                linear_wgrad=nothing, gemm=gemm, attention_fwd_ex=attn(torch.bfloat16), attention_fwd_ex_f16=attn(torch.float16),
                onequery_fwd=oneq(torch.bfloat16), onequery_fwd_f16=oneq(torch.float16), attention_bwd_ex=nothing, onequery_bwd=nothing,
                dropout_f32=nothing, dropout_bf16_=nothing)


@contextlib.contextmanager
def recording(st, fakes=None, recorder=Recorder):
    """fakes: op -> what stands in for it, for the set of ops a trace meets (default: the MED BERT's, RECORDED); recorder: the Recorder
    class (it finds the real functions as rec.real)"""
    from uniir_amd import ops
    if fakes is None:
        fakes = _fakes()
        assert set(fakes) == set(RECORDED)
    rec = recorder(st)
    rec.real = real = {n: getattr(ops, n) for n in fakes}
    try:
        for n in fakes:
            setattr(ops, n, rec.wrap(n, fakes[n]))
        yield rec
    finally:
        for n, fn in real.items():
            setattr(ops, n, fn)


def trace(case):
    """the entries of one case: bert_forward, then (bf16) bert_backward on the stash it kept"""
    from uniir_amd import blip_model as bm, flat_store, ops
    ff, half = case["model"] == "FF", case["dtype"] == "fp16"
    cfg = {**bm.MED_DEFAULT, **dict(hidden_size=W, intermediate_size=I, num_attention_heads=HEADS, num_hidden_layers=case["layers"],
                                    vocab_size=64, max_position_embeddings=16)}
    st = flat_store.FlatStore([("text_encoder." + n, s) for n, s in bm.bert_param_shapes(cfg, ENC, pooler=ff)], "cpu")
    dtype16 = torch.float16 if half else torch.bfloat16
    ids, key_len = torch.zeros(M, L, dtype=torch.int32), torch.tensor(KEY_LEN, dtype=torch.int32)
    img = torch.zeros(M * TI, ENC, dtype=dtype16) if ff else None
    pack = bm.TextPack.build(key_len, L) if case["pack"] else None
    assert (pack is not None) == case["pack"]
    torch.manual_seed(SEED)
    drop = ops.DropSeeds() if case["drop"] else None
    log = []
    with recording(st) as rec:
        out, stash = bm.bert_forward(st, "text_encoder.", cfg, ids, key_len, img, TI if ff else 0, not half, cross=ff, pool=ff, drop=drop,
                                     pack=pack, pool_last=case["pool_last"], log=log, dtype16=dtype16)
        assert out.dtype == torch.float32 and out.shape == (M, W) and (stash is None) == half
        rec.entries.append(["returned", rec.enc(out)])
        dimg = "no backward"
        if not half:
            dimg = bm.bert_backward(st, "text_encoder.", cfg, torch.zeros(M, W), stash, cross=ff, pool=ff)
            assert all(sv is None for sv in stash["layers"])          # the layer stash is released as the backward goes
            dimg = None if dimg is None else rec.enc(dimg)
    return rec.entries + [["log", log], ["dimg", dimg]]


FULL = ("bf16-FF-packed-pool_last-drop-2L",)          # the cases whose entries the fixture holds in full, next to every case's digests


def digest(entry):
    """ten hex digits of an entry's SHA-256: what the fixture holds of every entry of every case"""
    return hashlib.sha256(json.dumps(entry, separators=(",", ":"), sort_keys=True).encode()).hexdigest()[:10]


def first_difference(got, want_digests, want_full=None):
    """the first entry of the trace `got` whose digest is not the recorded one (with the recorded entry where the fixture has it)"""
    have = [digest(e) for e in got]
    for i, (g, w) in enumerate(zip(have, want_digests)):
        if g != w:
            was = "" if want_full is None else f"\n  recorded {json.dumps(want_full[i])}"
            return f"entry {i} of {len(got)} (digest {g}, recorded {w}):\n  got      {json.dumps(got[i])}{was}"
    if len(have) != len(want_digests):
        return f"{len(have)} entries, {len(want_digests)} recorded; the common part is equal"
    return None
