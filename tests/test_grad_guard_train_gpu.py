"""The gradient guard through the optimizer (trainer.NativeAdamW(max_grad_norm=..., skip_nonfinite=...)) on the tiny models of the
other GPU suites: clipping equals an unguarded step on the pre-multiplied gradient bit for bit, an out-of-range clip and a clean
step equal the unguarded step, a non-finite gradient skips every store's step and names its tensor, the step after a skipped one
uses bias correction 1, and two ranks skip together."""
import json
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))
ADAM = dict(lr=1e-3, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, allreduce=False)


@pytest.fixture(autouse=True)
def _no_guard_from_the_environment(monkeypatch):
    monkeypatch.delenv("UNIIR_MAX_GRAD_NORM", raising=False)
    monkeypatch.delenv("UNIIR_SKIP_NONFINITE", raising=False)


def _clip(seed=3, pairs=8):
    """the tiny CLIP_SF of tests/test_clip_model_gpu.py (width 64, 2 layers) and a device batch"""
    from oracle import clip_oracle as O
    from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
    from uniir_amd import clip_model
    cfg = O.tiny_config()
    clip_model.CLIP_CONFIGS["tiny-guard"] = cfg
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    model = CLIPScoreFusion("tiny-guard", device="cuda", config=config)
    model.clip_model.load_state_dict(O.init_state_dict(cfg, seed=seed), strict=True)
    model.train()
    batch = O.synthetic_batch(cfg, pairs, seed=5)
    return model, {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}


def _backward(model, opt, batch, **kw):
    opt.zero_grad()
    out = model(batch, **kw)
    opt.arm_overlap()
    out["loss"].backward()
    return out


def _stores(opt):
    return [opt.clip._ensure_flat()] + [e.store() for e in opt.extra]


def _snapshot(opt):
    """p32, bf16 shadow and both moments of every store, as bits"""
    opt._buffers()
    out = []
    for i, st in enumerate(_stores(opt)):
        m, v = opt._moments(i, st)
        out += [st.p32.clone(), st.w16_buf.view(torch.int16).clone(), m.clone(), v.clone()]
    return out


def _same(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x, y.view(torch.int32) if y.dtype == torch.float32 else y)
               for x, y in zip(a, b))


def _ref_sumsq(opt):
    """float64 torch sum of squares over the AdamW ranges of every store, and their element count"""
    total, n = 0.0, 0
    for st, ranges in opt._ranges:
        for lo, hi, _ in ranges:
            total += float((st.g32[lo:hi].double() ** 2).sum())
            n += hi - lo
    return total, n


def _twin_with_gradients_of(model_opt, seed=3, **kw):
    from uniir_amd.trainer import NativeAdamW
    twin, _ = _clip(seed)
    opt = NativeAdamW(twin.clip_model, **ADAM, **kw)
    opt.zero_grad()
    twin.clip_model._ensure_flat().g32.copy_(model_opt.clip._ensure_flat().g32)
    return twin, opt


def test_clipping_equals_an_unguarded_step_on_the_scaled_gradient():
    from uniir_amd.trainer import NativeAdamW
    model, batch = _clip()
    opt = NativeAdamW(model.clip_model, **ADAM, max_grad_norm=0.05)
    _backward(model, opt, batch)
    twin, topt = _twin_with_gradients_of(opt)
    assert _same(_snapshot(opt), _snapshot(topt))
    opt.step()
    stats = opt.grad_stats()
    # the norm against a float64 torch norm: the device's sum and torch's are each within n * 2^-53 of the exact sum of squares, the
    # root halves a relative error, and the result is rounded to fp32 once
    ref, n = _ref_sumsq(opt)
    print(f"\nOBS guard train: norm {stats['norm']!r} torch f64 {ref ** 0.5!r} coef {stats['coef']!r} n {n}")
    assert abs(stats["sumsq"] - ref) <= 2 * n * 2.0 ** -53 * ref
    assert abs(stats["norm"] - ref ** 0.5) <= ref ** 0.5 * (n * 2.0 ** -53 + 2.0 ** -24)
    coef = np.float32(0.05) / (np.float32(stats["norm"]) + np.float32(1e-6))
    assert stats["coef"] == float(coef) and 0 < stats["coef"] < 1, "max_grad_norm 0.05 was meant to clip"
    assert not stats["skipped"] and stats["first_bad"] is None and (stats["steps_seen"], stats["steps_skipped"]) == (1, 0)
    # the twin: its gradient times the coefficient in fp32, then the plain step
    twin.clip_model._ensure_flat().g32.mul_(float(coef))
    topt.step()
    torch.cuda.synchronize()
    assert topt.guard is None and _same(_snapshot(opt), _snapshot(topt))
    assert opt.opt_step == topt.opt_step == 1


def test_clipping_out_of_range_and_a_clean_skip_guard_equal_the_unguarded_step():
    from uniir_amd.trainer import NativeAdamW
    for kw in (dict(max_grad_norm=1e30), dict(skip_nonfinite=True), dict(max_grad_norm=1e30, skip_nonfinite=True)):
        model, batch = _clip()
        opt = NativeAdamW(model.clip_model, **ADAM, **kw)
        _backward(model, opt, batch)
        twin, topt = _twin_with_gradients_of(opt)
        before = _snapshot(opt)
        opt.step()
        topt.step()
        torch.cuda.synchronize()
        assert _same(_snapshot(opt), _snapshot(topt)) and not _same(_snapshot(opt), before)
        stats = opt.grad_stats()
        assert stats["coef"] == 1.0 and not stats["skipped"] and stats["norm"] > 0


def test_nonfinite_gradient_skips_the_step_and_the_next_one_counts_from_one():
    from uniir_amd.trainer import NativeAdamW
    model, batch = _clip()
    opt = NativeAdamW(model.clip_model, **ADAM, skip_nonfinite=True, max_grad_norm=1e30)
    _backward(model, opt, batch)
    st = opt.clip._ensure_flat()
    names = list(st.off)
    name = names[len(names) // 2]
    before = _snapshot(opt)
    st.grad_view(name).view(-1)[-1] = float("nan")
    opt.step()
    assert opt.opt_step == 1                                       # nothing was read back inside step()
    stats = opt.grad_stats()
    assert _same(_snapshot(opt), before), "a skipped step moved something"
    assert stats["skipped"] and stats["nonfinite"] and stats["coef"] == 0.0 and stats["first_bad"] == name
    assert (stats["steps_seen"], stats["steps_skipped"]) == (1, 1) and opt.opt_step == 0
    # the next, clean step against a twin that never saw the bad one
    _backward(model, opt, batch)
    twin, topt = _twin_with_gradients_of(opt)
    opt.step()
    topt.step()
    torch.cuda.synchronize()
    assert _same(_snapshot(opt), _snapshot(topt)), "bias correction did not use step 1"
    stats = opt.grad_stats()
    assert not stats["skipped"] and stats["first_bad"] is None and (stats["steps_seen"], stats["steps_skipped"]) == (2, 1)
    assert opt.opt_step == topt.opt_step == 1
    sd = opt.state_dict()
    assert (sd["opt_step"], sd["steps_seen"], sd["steps_skipped"]) == (1, 2, 1)
    # +Inf is as bad as NaN, and the counters were restored: a fresh optimizer continues them on the device
    fresh = NativeAdamW(model.clip_model, **ADAM, skip_nonfinite=True)
    fresh.load_state_dict(sd)
    _backward(model, fresh, batch)
    st.grad_view(names[0]).view(-1)[0] = float("inf")
    before = _snapshot(fresh)
    fresh.step()
    stats = fresh.grad_stats()
    assert _same(_snapshot(fresh), before) and stats["first_bad"] == names[0]
    assert (stats["steps_seen"], stats["steps_skipped"], fresh.opt_step) == (3, 2, 1)


def test_without_skip_a_nonfinite_gradient_is_reported_and_applied():
    """max_grad_norm alone does not skip: the step goes through unclipped, as clip_grad_norm_ followed by optimizer.step() would"""
    from uniir_amd.trainer import NativeAdamW
    model, batch = _clip()
    opt = NativeAdamW(model.clip_model, **ADAM, max_grad_norm=0.05)
    _backward(model, opt, batch)
    st = opt.clip._ensure_flat()
    name = list(st.off)[1]
    st.grad_view(name).view(-1)[0] = float("nan")
    opt.step()
    stats = opt.grad_stats()
    assert stats["nonfinite"] and not stats["skipped"] and stats["coef"] == 1.0 and stats["first_bad"] == name
    assert torch.isnan(st.p(name).view(-1)[0]) and opt.opt_step == 1


def test_clipff_norm_covers_both_stores_and_a_t5_nan_skips_clip_too():
    from oracle import clip_oracle as O
    from models.uniir_clip.clip_featurefusion.clip_ff import CLIPFeatureFusion
    from uniir_amd import clip_model
    from uniir_amd.trainer import NativeAdamW
    t5_cfg = dict(d_model=128, num_heads=2, d_ff=256, num_layers=2)          # the small geometry of tests/test_clipff_gpu.py
    cfg = O.tiny_config(embed_dim=128, transformer_width=128, transformer_heads=2)
    clip_model.CLIP_CONFIGS["tiny-ff-guard"] = cfg
    config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
    m = CLIPFeatureFusion("tiny-ff-guard", device="cuda", config=config, t5_config=dict(dropout_rate=0.0, **t5_cfg))
    sd = O.init_state_dict(cfg, seed=5)
    sd.pop("text_projection")
    m.clip_model.load_state_dict(sd, strict=True)
    m.train()
    batch = O.synthetic_batch(cfg, 4, seed=23)
    batch = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
    opt = NativeAdamW(m.clip_model, lr=1e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.2, allreduce=False,
                      extra=[m.t5_optimizer_group(lr=1e-3)], max_grad_norm=1e30, skip_nonfinite=True)
    _backward(m, opt, batch)
    before = _snapshot(opt)
    opt.step()
    stats = opt.grad_stats()
    ref, n = _ref_sumsq(opt)
    per_store = [sum(float((st.g32[lo:hi].double() ** 2).sum()) for lo, hi, _ in rs) for st, rs in opt._ranges]
    assert len(per_store) == 2 and min(per_store) > 0
    assert abs(stats["sumsq"] - ref) <= 2 * n * 2.0 ** -53 * ref and stats["sumsq"] > max(per_store) * (1 + 1e-9)
    assert abs(stats["norm"] - ref ** 0.5) <= ref ** 0.5 * (n * 2.0 ** -53 + 2.0 ** -24)
    after = _snapshot(opt)
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[4], before[4])          # both stores stepped
    # a NaN in a T5 tensor: neither store moves
    _backward(m, opt, batch)
    t5 = opt.extra[0].store()
    name = list(t5.off)[3]
    t5.grad_view(name).view(-1)[1] = float("nan")
    before = _snapshot(opt)
    opt.step()
    stats = opt.grad_stats()
    assert _same(_snapshot(opt), before) and stats["skipped"] and stats["first_bad"] == name
    assert (stats["steps_seen"], stats["steps_skipped"], opt.opt_step) == (2, 1, 1)


def test_blip_ff_skipped_step_leaves_the_online_store_and_keeps_the_forward_s_queues():
    from uniir_amd.blip_model import BLIPFeatureFusion
    from uniir_amd.trainer import NativeAdamW
    z = np.load(os.path.join(GOLD, "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    model = BLIPFeatureFusion(med_config=med_cfg, vit_config=vit_cfg, embed_dim=med_cfg["hidden_size"], queue_size=16, momentum=0.9,
                              config=types.SimpleNamespace(tokenizer_max_length=20)).cuda()
    model.train()
    opt = NativeAdamW(model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05, allreduce=False, skip_nonfinite=True)
    b = 4
    batch = {
        "txt_batched": types.SimpleNamespace(input_ids=torch.from_numpy(z["s0_ids"]).cuda(),
                                             attention_mask=torch.from_numpy(z["s0_mask"]).cuda()),
        "image_batched": torch.from_numpy(z["s0_img"]).cuda(),
        "p_did_list": torch.from_numpy(z["s0_pdid"]),
        "index_mapping": {"query": [[2 * i] for i in range(b)], "pos_cand": [[2 * i + 1] for i in range(b)]},
    }
    queues0 = [t.clone() for t in (model.query_queue, model.cand_queue, model.idx_queue)]
    _backward(model, opt, batch, alpha=0.4)
    before = _snapshot(opt)
    forward_left = [t.clone() for t in (model.query_queue, model.cand_queue, model.idx_queue, model._mom.p32)]
    assert not torch.equal(forward_left[0], queues0[0])                       # the forward did enqueue
    name = "text_encoder.pooler.dense.weight"
    model.get_parameter(name).grad.view(-1)[7] = float("nan")
    opt.step()
    stats = opt.grad_stats()
    assert stats["skipped"] and stats["first_bad"] == name and (stats["steps_seen"], stats["steps_skipped"]) == (1, 1)
    assert _same(_snapshot(opt), before), "the online store moved on a skipped step"
    now = [model.query_queue, model.cand_queue, model.idx_queue, model._mom.p32]
    assert all(torch.equal(a, b_) for a, b_ in zip(now, forward_left)), "queues / momentum weights lost what the forward did"
    # and the next step is applied
    _backward(model, opt, batch, alpha=0.4)
    opt.step()
    stats = opt.grad_stats()
    assert not stats["skipped"] and opt.opt_step == 1 and not _same(_snapshot(opt), before)


# ---- two ranks on one GPU (the harness of tests/test_dist_device_gpu.py) --------------------------------------------------------
def _rank_worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
        os.environ.pop("UNIIR_MAX_GRAD_NORM", None)
        os.environ.pop("UNIIR_SKIP_NONFINITE", None)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "uniir_amd", "src"))
        from oracle import clip_oracle as O
        from models.uniir_clip.clip_scorefusion.clip_sf import CLIPScoreFusion
        from uniir_amd import clip_model
        from uniir_amd.trainer import NativeTrainer
        cfg = O.tiny_config()
        clip_model.CLIP_CONFIGS["tiny-guard-dist"] = cfg
        config = SimpleNamespace(model=SimpleNamespace(gather_embeddings=False), data_config=SimpleNamespace(in_batch_neg_num=0))
        model = CLIPScoreFusion("tiny-guard-dist", device="cuda:0", config=config)
        model.clip_model.load_state_dict(O.init_state_dict(cfg, seed=9))
        tr = NativeTrainer(model, lr=1e-3, t_total=10, skip_nonfinite=True)
        pairs = 4
        full = O.synthetic_batch(cfg, 2 * pairs, seed=31)
        lo, hi = rank * 2 * pairs, (rank + 1) * 2 * pairs
        batch = {k: (v[lo:hi].cuda() if isinstance(v, torch.Tensor) else v) for k, v in full.items()}
        batch["index_mapping"] = {"query": [[2 * i] for i in range(pairs)], "pos_cand": [[2 * i + 1] for i in range(pairs)]}
        bad = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in batch.items()}
        if rank == 1:                                                  # only this rank's batch is corrupt
            bad["image_batched"].view(-1)[5] = float("nan")
        p32 = model.clip_model._ensure_flat().p32
        init = p32.cpu().numpy().copy()
        loss_bad = float(tr.train_step(bad)["loss"].detach())
        s1 = dict(tr.opt.grad_stats())
        after_bad = p32.cpu().numpy().copy()
        tr.train_step(batch)
        s2 = dict(tr.opt.grad_stats())
        after_good = p32.cpu().numpy().copy()
        q.put((rank, None, loss_bad, s1, s2, np.array_equal(init.view(np.int32), after_bad.view(np.int32)), after_good,
               tr.opt.opt_step, tr.sched.step_count))
        dist.barrier()
        dist.destroy_process_group()
    except Exception as e:          # the parent must not wait for its queue timeout
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))


def test_two_ranks_skip_together_and_apply_the_next_step():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, 29571, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=240) for _ in range(2)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
    for r in res:
        assert r[1] is None, r[1]
    (_, _, l0, a1, a2, same0, w0, step0, sched0), (_, _, l1, b1, b2, same1, w1, step1, sched1) = res
    assert np.isfinite(l0) and not np.isfinite(l1)                     # only rank 1's batch produced the NaN
    assert a1["skipped"] and b1["skipped"] and same0 and same1         # both skipped, nothing moved
    assert a1["first_bad"] == b1["first_bad"] is not None
    assert not a2["skipped"] and not b2["skipped"]
    assert (a2["steps_seen"], a2["steps_skipped"]) == (b2["steps_seen"], b2["steps_skipped"]) == (2, 1)
    assert np.array_equal(w0.view(np.int32), w1.view(np.int32))        # the replicas stay identical
    assert step0 == step1 == 1 and sched0 == sched1 == 2               # one applied step; the scheduler advanced on both
    assert a2["norm"] == b2["norm"] and a2["norm"] > 0
