"""Why tests/test_clipff_336_gpu.py may hold the 654-token model to the gates of tests/test_clipff_gpu.py, shown on the CPU with the
oracle alone: oracle/clipff_oracle.py under torch.autocast("cpu", bfloat16) -- bf16 operands in every product, no kernel of this
project -- against the same computation in fp32, on the tiny model, batch, token features and dropout masks of that test.  The bf16
run meets every gate with at least a factor two to spare (relative L2 below half the gate; for the direction, 1 - cosine below half of
1 - 0.985) with the q projections at transformers' T5 initialisation (Q_GAIN of that test), and misses that room at the module's own
(gain 1: unit-variance q and k, un-scaled logits of standard deviation 8) -- the gates are a statement about the arithmetic with room
for a kernel only at Q_GAIN, which is why the GPU test scales q and does not widen a gate."""
import torch

import test_clipff_336_gpu as T
from test_clipff_gpu import cos, rel

SPARE = 2.0


def _deep_with_room(a, b, what):
    assert (1.0 - cos(a, b)) * SPARE < 1.0 - 0.985 and rel(a, b) * SPARE < 0.2, (what, cos(a, b), rel(a, b))


def _step_figures(q_gain):
    m, sd, cfg = T.build("cpu", q_gain=q_gain)
    batch = T.batch_of(cfg)
    t5 = T.t5_state(m)
    _, _, g32 = T.oracle_step(sd, t5, cfg, batch)
    _, _, g16 = T.oracle_step(sd, t5, cfg, batch, bf16=True)
    return max(rel(g16[n], g32[n]) for n in g32), min(cos(g16[n], g32[n]) for n in g32)


def test_at_gain_1_the_oracle_in_bf16_has_less_than_that_room():
    worst_rel, worst_cos = _step_figures(1.0)
    print(f"\nOBS clipff-336 oracle bf16 against fp32 at q gain 1: worst gradient rel {worst_rel:.4f} cos {worst_cos:.4f}")
    assert worst_rel * SPARE > 0.2 or (1.0 - worst_cos) * SPARE > 1.0 - 0.985          # measured 0.108, 0.9943


def test_the_oracle_in_bf16_meets_the_gates_of_the_training_step_with_room():
    m, sd, cfg = T.build("cpu")
    batch = T.batch_of(cfg)
    t5 = T.t5_state(m)
    emb32, out32, g32 = T.oracle_step(sd, t5, cfg, batch)
    emb16, out16, g16 = T.oracle_step(sd, t5, cfg, batch, bf16=True)
    print(f"\nOBS clipff-336 oracle bf16 against fp32: emb {rel(emb16, emb32):.4g} loss {out16['loss'].item():.5f} / {out32['loss'].item():.5f}")
    print("OBS clipff-336 oracle bf16 gradients (cos, rel):", {n[-36:]: (round(cos(g16[n], g32[n]), 4), round(rel(g16[n], g32[n]), 4)) for n in g32})
    assert rel(emb16, emb32) * SPARE < 2e-2
    assert abs(out16["loss"].item() - out32["loss"].item()) * SPARE < 3e-2 * max(1.0, abs(out32["loss"].item()))
    for n in g32:
        _deep_with_room(g16[n], g32[n], n)


def test_the_oracle_in_bf16_meets_the_gates_of_the_dropout_step_with_room():
    m, _, _ = T.build("cpu", dropout_rate=T.DROP_P)
    t5 = T.t5_state(m)
    txt, img, w = T.fusion_inputs()

    def masks_from(seed):
        g = torch.Generator().manual_seed(seed)
        return lambda kind, shape: (torch.rand(shape, generator=g) >= T.DROP_P).float() / (1.0 - T.DROP_P)

    p32, dx32, g32 = T.oracle_dropout_step(t5, txt, img, w, masks_from(3))
    p16, dx16, g16 = T.oracle_dropout_step(t5, txt, img, w, masks_from(3), bf16=True)
    print(f"\nOBS clipff-336 oracle bf16 against fp32, dropout step: pooled {rel(p16, p32):.4g} dx (cos, rel) {cos(dx16, dx32):.4f} {rel(dx16, dx32):.4f}")
    print("OBS clipff-336 oracle bf16 dropout gradients (cos, rel):", {n[-36:]: (round(cos(g16[n], g32[n]), 4), round(rel(g16[n], g32[n]), 4)) for n in g32})
    assert rel(p16, p32) * SPARE < 2e-2
    _deep_with_room(dx16, dx32, "dx")
    for n in g32:
        _deep_with_room(g16[n], g32[n], n)
