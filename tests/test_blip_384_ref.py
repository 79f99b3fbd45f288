"""Why tests/test_blip_384_gpu.py judges its contrastive step at BASE_GAIN and not at the model's own initialisation, shown on the CPU
with the oracle alone: oracle/blip_oracle.py's contrastive step under torch.autocast("cpu", bfloat16) -- bf16 operands in every product,
no kernel of this project -- against the same step in fp32, on the tiny 384-pixel model, batch and queues of that test.  At gain 1 the
sampled gradients of the bf16 run miss the gate the GPU test applies (8e-2) by a wide margin; at BASE_GAIN they are inside it.  The
gate is therefore a statement about the arithmetic only at BASE_GAIN."""
import torch

import test_blip_384_gpu as T


def _worst(gain):
    model = T.tiny_model(gain=gain)
    sd0 = {n: p.detach().clone() for n, p in model.named_parameters()}
    ids, mask, img = T._inputs()
    res = []
    for bf16 in (False, True):
        sd = {n: v.clone() for n, v in sd0.items()}
        qq, cq, iq = T._queues(model.queue_size)
        state = {"query_queue": qq, "cand_queue": cq, "idx_queue": iq, "ptr": 0}
        with torch.autocast("cpu", dtype=torch.bfloat16, enabled=bf16):
            T._oracle_step(sd, ids, mask, img, state, model.vit_cfg, model.med_cfg)
        res.append({n: sd[n].grad for n in T.GRADS})
    errs = {n: T.rel(res[1][n], res[0][n]) for n in T.GRADS}
    print(f"\nOBS blip-384 oracle bf16 against fp32, gain {gain}:", {k[-40:]: round(v, 4) for k, v in errs.items()})
    return max(errs.values())


def test_the_oracle_in_bf16_misses_the_gradient_gate_at_gain_1_and_meets_it_at_base_gain():
    assert _worst(1.0) > 2 * 8e-2            # measured 0.25
    assert _worst(T.BASE_GAIN) < 8e-2        # measured 0.027
