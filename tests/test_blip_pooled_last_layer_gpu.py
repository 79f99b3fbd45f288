"""BLIPFeatureFusion.pool_last_layer (UNIIR_BLIP_POOL_LAST_LAYER=1): the last BERT layer on the class row of every caption -- the
one-query attention with key counts, packed keys and dropout (uniir_onequery_fwd / _bwd) and everything behind the q | k | v projection
on M rows -- against the full layer on the same weights, tokens, images and dropout seeds.  Tiny BLIP configurations with the shapes of
the goldens g6 / g8 / g8s (tests/test_blip_gpu.py), hidden and attention dropout 0.1 in train mode, captions of length 1 and of full
length in the batch:
  bit for bit: the eval embeddings (with grad, without, and the momentum encoder's), the train-mode output, the loss of a training step;
  parameter gradients by relative L2 norm per parameter under the gates of tests/test_pooled_long_gpu.py for the same mechanism: 1e-5
  (the order of fp32 sums) for the parameters whose gradient does not pass through an attention backward of the pooled layer -- what
  lies behind its last attention: output.*, intermediate.*, the pooler / text_proj, and crossattention.output.* (BLIP_FF) or
  attention.output.* (BLIP_SF); their linear biases 2^-7 below 256 rows, as there: one form sums a bias gradient from the rounded bf16
  result, the other from the fp32 accumulators -- and 1e-2 for everything upstream of it (the full layer runs the tiled attention
  backward, which rounds P and dS to bf16; the one-pass kernel keeps them in fp32).  The attention key biases, whose gradient is
  analytically zero, are judged inside the fused [q | k | v] / [k | v] bias vectors (_fuse_key_biases says why);
  the oracle gates of test_g6_med_bert_forward_backward and test_blip_ff_train_mode_dropout_matches_masked_oracle with the flag on;
  two flag-on training steps bit for bit equal; the path log says that the pooled layer ran."""
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

import test_blip_gpu as TB

pytestmark = pytest.mark.gpu
G = TB.G


def _model(score_fusion, layers, seed=11):
    from uniir_amd.blip_model import BLIPFeatureFusion, BLIPScoreFusion
    z = np.load(os.path.join(G, "g8s_blipsf.npz" if score_fusion else "g8_blipff.npz"))
    med_cfg, vit_cfg = json.loads(str(z["med_cfg"])), json.loads(str(z["vit_cfg"]))
    med_cfg.update(num_hidden_layers=layers, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    cls = BLIPScoreFusion if score_fusion else BLIPFeatureFusion
    embed = int(z["embed_dim"]) if score_fusion else med_cfg["hidden_size"]
    model = cls(med_config=med_cfg, vit_config=vit_cfg, embed_dim=embed, queue_size=16, momentum=0.9,
                config=types.SimpleNamespace(tokenizer_max_length=20), seed=seed).cuda()
    ids = torch.from_numpy(z["s0_ids"]).clone()
    M, L = ids.shape
    lens = torch.tensor([(L, 1, L // 2 + 1, 2, L - 1, 3)[m % 6] for m in range(M)])          # full length, one token, ragged
    mask = (torch.arange(L).unsqueeze(0) < lens.unsqueeze(1)).long()
    ids = ids * mask
    img = torch.from_numpy(z["s0_img"]).cuda()
    pdid = torch.from_numpy(z["s0_pdid"])
    return model, ids, mask, img, pdid


def _own(name, layers, cross):
    """parameters whose gradient does not pass through an attention backward of the pooled layer: behind its last attention -- the
    cross-attention in BLIP_FF (attention.output.* lies upstream of it there), the self-attention in BLIP_SF"""
    last = f"text_encoder.encoder.layer.{layers - 1}."
    subs = ("output.", "intermediate.", "crossattention.output.") if cross else ("output.", "intermediate.", "attention.output.")
    return name.startswith(("text_encoder.pooler.", "text_proj.")) or (name.startswith(last) and name[len(last):].startswith(subs))


def _fuse_key_biases(g):
    """The key bias of an attention has NO gradient: sum_j dS[i][j] = sum_j p_j f_j dP_j - D_i sum_j p_j = D_i - D_i = 0 for every
    query row, so d key.bias = scale sum_i q_i sum_j dS[i][j] = 0, and what either form holds there is the rounding residue of a sum that
    cancels -- a relative error against it measures nothing.  It is judged as the kernels hold it: as a part of the adjacent [q | k | v]
    (self) and [k | v] (cross) bias vectors that one weight-gradient GEMM accumulates (blip_model.bert_param_shapes), the unit that CLIP's
    in_proj_bias is in tests/test_pooled_long_gpu.py.  -> the fused dict, and the key biases on their own (printed only)"""
    out, keys = {}, {}
    for n, t in g.items():
        if n.endswith(("attention.self.key.bias", "attention.self.value.bias")):          # (matches crossattention.self.* too)
            continue
        if n.endswith("crossattention.self.query.bias") or not n.endswith("attention.self.query.bias"):
            out[n] = t
    for n, t in g.items():
        if n.endswith("attention.self.key.bias"):
            base = n[:-len("key.bias")]
            keys[n] = t
            cross = base.endswith("crossattention.self.")
            parts = ([] if cross else [g[base + "query.bias"]]) + [t, g[base + "value.bias"]]
            out[base + ("[k|v]" if cross else "[q|k|v]") + ".bias"] = torch.cat([x.flatten() for x in parts])
    return out, keys


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "dense"])
@pytest.mark.parametrize("score_fusion", [False, True], ids=["ff", "sf"])
def test_pooled_last_layer_equals_the_full_layer(score_fusion, packed, layers):
    model, ids, mask, img, _ = _model(score_fusion, layers)
    model.pack_text = packed
    M = ids.shape[0]
    w = torch.randn(M, model.embed_dim, generator=torch.Generator().manual_seed(5)).cuda()

    def run(flag, train):
        model.pool_last_layer = flag
        model.train(train)
        model.zero_grad()
        n_log = len(model.path_log)
        txt = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
        torch.manual_seed(21)
        emb = model.encode_multimodal_input(txt, img)
        assert model.last_text_rows == ((int(mask.sum()) if packed else ids.numel()), ids.numel())
        (emb * w).sum().backward()
        grads = {n: p.grad.detach().clone() for n, p in model._online_params() if n not in model._frozen and n != "temp"}
        with torch.no_grad():
            torch.manual_seed(22)
            emb_m = model.encode_multimodal_input(txt, img, use_momentum=True)
            torch.manual_seed(23)
            emb_n = model.encode_multimodal_input(txt, img)
        new = model.path_log[n_log:]
        if flag:          # the online pass with its stash, the momentum pass, the no-grad pass
            assert len(new) == 3 and all("class rows" in x and "pool_last_layer" in x for x in new), new
            assert "stash of M-row tensors" in new[0] and "no stash" in new[1] and "no stash" in new[2], new
            assert all(("packed" if packed else "dense") in x and (("self- and cross-" in x) != score_fusion) for x in new), new
        else:
            assert not new, new
        return emb.detach().clone(), emb_m.clone(), emb_n.clone(), grads

    for train in (False, True):
        e_f, m_f, n_f, g_f = run(False, train)
        e_p, m_p, n_p, g_p = run(True, train)
        assert torch.equal(e_p, e_f), (train, float((e_p - e_f).abs().max()))
        assert torch.equal(m_p, m_f), (train, float((m_p - m_f).abs().max()))
        assert torch.equal(n_p, n_f), (train, float((n_p - n_f).abs().max()))
        if train:
            assert not torch.equal(e_f, n_f)          # other seeds, other masks: dropout did something
        worst = {True: (0.0, ""), False: (0.0, "")}
        bad = []
        (g_f, k_f), (g_p, k_p) = _fuse_key_biases(g_f), _fuse_key_biases(g_p)
        assert len(k_f) == layers * (1 if score_fusion else 2)
        print("\nOBS key biases (no gradient: rounding residue) |flag off|, |flag on|, |fused vector|: " + "; ".join(
            f"{n[len('text_encoder.encoder.'):]} {float(k_f[n].norm()):.3g} {float(k_p[n].norm()):.3g} "
            f"{float(g_f[n[:-len('key.bias')] + ('[k|v]' if 'cross' in n else '[q|k|v]') + '.bias'].norm()):.3g}" for n in k_f))
        for n in g_f:
            err = float((g_p[n] - g_f[n]).norm() / g_f[n].norm().clamp_min(1e-20))
            own = _own(n, layers, not score_fusion)
            gate = 1e-5 if own else 1e-2
            if own and M < 256 and n.endswith("bias") and "LayerNorm" not in n:
                gate = 2.0 ** -7
            worst[own] = max(worst[own], (err, n))
            if not err <= gate:
                bad.append((n, err, gate))
        print(f"\nOBS blip pooled last layer vs full, {'sf' if score_fusion else 'ff'} {'packed' if packed else 'dense'} {layers} layers "
              f"train={train}: worst own {worst[True]}, worst upstream {worst[False]}")
        assert not bad, bad
        assert sum(float(g_f[n].abs().max()) > 0 for n in g_f) >= len(g_f) - (4 if score_fusion else 0)


def _step(score_fusion, packed, flag):
    """one training step (train mode, dropout on) from a fixed state -> loss, gradients, momentum weights, queues"""
    model, ids, mask, img, pdid = _model(score_fusion, 2)
    model.copy_params()
    model.pack_text, model.pool_last_layer = packed, flag
    model.train()
    torch.manual_seed(77)
    b = len(pdid)
    batch = {"txt_batched": types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda()), "image_batched": img,
             "p_did_list": pdid, "index_mapping": {"query": [[2 * i] for i in range(b)], "pos_cand": [[2 * i + 1] for i in range(b)]}}
    model.zero_grad()
    out = model(batch, alpha=0.4)
    out["loss"].backward()
    torch.cuda.synchronize()
    assert bool(model.path_log) == flag
    return (out["loss"].detach().clone(), model._online.g32.clone(), model._mom.p32.clone(), model.query_queue.clone(),
            model.cand_queue.clone())


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "dense"])
@pytest.mark.parametrize("score_fusion", [False, True], ids=["ff", "sf"])
def test_training_step_same_loss_and_two_flag_on_steps_bit_for_bit(score_fusion, packed):
    off, on1, on2 = (_step(score_fusion, packed, flag) for flag in (False, True, True))
    assert torch.equal(on1[0], off[0]), (float(on1[0]), float(off[0]))
    for k in (3, 4):          # what was enqueued: the momentum features
        assert torch.equal(on1[k], off[k]), k
    for k, (a, b) in enumerate(zip(on1, on2)):
        assert torch.equal(a, b), (k, int((a != b).sum()), float((a.float() - b.float()).abs().max()))


def test_g6_oracle_gates_with_the_flag_on(monkeypatch):
    from uniir_amd import blip_model as bm
    log = []
    monkeypatch.setattr(bm, "bert_forward", functools.partial(bm.bert_forward, pool_last=True, log=log))
    TB.test_g6_med_bert_forward_backward()
    assert len(log) == 1 and "class rows" in log[0], log


def test_masked_oracle_gates_with_the_flag_on(monkeypatch):
    from uniir_amd import ops
    calls = []
    orig = ops.onequery_fwd

    def spy(*a, **k):
        calls.append(1)
        return orig(*a, **k)

    monkeypatch.setattr(ops, "onequery_fwd", spy)          # a last layer on the class rows: its self- and its cross-attention
    monkeypatch.setenv("UNIIR_BLIP_POOL_LAST_LAYER", "1")
    TB.test_blip_ff_train_mode_dropout_matches_masked_oracle()
    assert len(calls) >= 2 * 4, calls          # two eval passes, the training pass, the no-grad pass
