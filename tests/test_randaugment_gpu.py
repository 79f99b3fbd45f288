"""BLIP's RandomAugment on the device (uniir_image_aug_plan + uniir_image_augment_batch / uniir_image_preprocess_batch_aug,
clip_front.augment_batch_on_device / PackedImages / RawImageBatch, blip_front.RawBlipTransform(randaugment=...)).  Every
comparison is exact: the op kernels against the numpy restatement (tests/randaugment_ref.py, itself pinned by
tests/test_randaugment_ref.py) byte for byte, the full pipeline against the host transform bit for bit."""
import os
import random

import numpy as np
import pytest
import torch

import image_batch_cases as K
import randaugment_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# every op alone, both signs; level-5 arguments of the shipped recipe and general ones
SINGLE_OPS = [("Identity", 0.0), ("AutoContrast", 0.0), ("AutoContrastPIL", 0.0), ("Equalize", 0.0), ("Brightness", 0.1),
              ("Brightness", 0.64), ("Brightness", 1.0), ("Brightness", 1.9), ("Sharpness", 1.0), ("Sharpness", 0.0), ("Sharpness", 0.64),
              ("Sharpness", 1.9), ("ShearX", 0.15), ("ShearX", -0.15), ("ShearY", 0.15), ("ShearY", -0.15), ("ShearX", 0.24000000000000002),
              ("TranslateX", 5.0), ("TranslateX", -5.0), ("TranslateY", 5.0), ("TranslateY", -5.0), ("TranslateY", 2.3), ("Rotate", 15.0),
              ("Rotate", -15.0), ("Rotate", 24.0), ("Rotate", 180.0), ("TranslateX", 15.75 / 1024)]


def _device_ops(imgs, ops_per_image):
    from uniir_amd import clip_front
    x = torch.from_numpy(np.stack(imgs)).to(DEV)
    out, info = clip_front.augment_batch_on_device(x, ops_per_image)
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), torch.from_numpy(np.stack(imgs)))           # the input buffer is never written
    return out.cpu().numpy(), info


def _compare(imgs, ops_per_image, got):
    for i, (img, ops) in enumerate(zip(imgs, ops_per_image)):
        want = R.apply_ops(img, ops or [])
        assert np.array_equal(got[i], want), (i, ops, int(np.abs(got[i].astype(int) - want.astype(int)).max()))


@pytest.mark.parametrize("where", ["first", "last"])
@pytest.mark.parametrize("n", [16, 19, 24, 32])
def test_every_op_alone_equals_the_restatement(n, where):
    """one batch with one image per op: the op in the first slot of one, or in the last of four (Identity before it)"""
    imgs = [K.image(n, n, 300 + i) if i % 2 else R.smooth_image(n, amp=(100.0 - i, -80.0, 60.0 + i)) for i in range(len(SINGLE_OPS))]
    imgs[1][0, 0] = 0                                        # a channel minimum of 0: the one case AutoContrast stretches
    lists = [[op] if where == "first" else [("Identity", 0.0)] * 3 + [op] for op in SINGLE_OPS]
    got, info = _device_ops(imgs, lists)
    assert info.slots == (1 if where == "first" else 4) and info.launches == 2 * info.slots
    _compare(imgs, lists, got)
    assert not np.array_equal(got[SINGLE_OPS.index(("Rotate", 15.0))], imgs[SINGLE_OPS.index(("Rotate", 15.0))])


@pytest.mark.parametrize("n", [16, 19])
def test_table_edge_cases_of_the_fixture(n):
    """every image of G18 (min 0 / max 255, min > 0, max < 255, flat, two values, equalize's step 0) under every table op; the
    AutoContrast and Equalize bytes are also the reference's own (the fixture)"""
    g18 = np.load(os.path.join(os.path.dirname(__file__), "golden", "g18_randaugment.npz"))
    cases = {k: v for k, v in R.lut_cases().items() if v.shape[0] == n}
    assert len(cases) == 6
    ops = [("AutoContrast", 0.0), ("Equalize", 0.0), ("AutoContrastPIL", 0.0), ("Brightness", 0.1), ("Brightness", 0.64), ("Brightness", 1.9)]
    names = [k for k in cases for _ in ops]
    imgs = [cases[k] for k in names]
    lists = [[op] for _ in cases for op in ops]
    got, _ = _device_ops(imgs, lists)
    _compare(imgs, lists, got)
    for i, (k, (op,)) in enumerate(zip(names, lists)):
        if op[0] in ("AutoContrast", "Equalize"):
            assert np.array_equal(got[i], g18[f"{k}_{op[0].lower()}"]), (k, op)


def _mixed(n=24):
    imgs = [K.image(n, n, 500 + i) for i in range(7)]
    imgs[2] = R.smooth_image(n)
    lists = [[("Rotate", 15.0), ("Equalize", 0.0)],                  # warp, then statistics
             [("Identity", 0.0), ("Identity", 0.0)],                 # nothing at all
             [("AutoContrastPIL", 0.0), ("ShearX", -0.15)],          # statistics, then warp
             [("Sharpness", 0.64), ("Identity", 0.0)],
             None,                                                   # no list: Identity
             [("Equalize", 0.0), ("AutoContrast", 0.0)],             # statistics in both slots
             [("TranslateY", -5.0), ("Brightness", 1.54)]]
    return imgs, lists


def test_mixed_batch_of_seven_and_of_one():
    imgs, lists = _mixed()
    got, info7 = _device_ops(imgs, lists)
    _compare(imgs, lists, got)
    assert np.array_equal(got[1], imgs[1]) and np.array_equal(got[4], imgs[4])
    for i in (0, 2, 5):
        one, info1 = _device_ops(imgs[i:i + 1], lists[i:i + 1])
        assert np.array_equal(one[0], got[i]), i
        assert info1.launches == info7.launches == 4
    again, _ = _device_ops(imgs, lists)
    assert np.array_equal(again, got)


def test_all_identity_table_equals_the_plain_entry_point():
    """image_batch_cases.mixed_batch(16) scattered into 10 slots: the _aug entry with an all-Identity table == the plain entry
    under torch.equal, and the slots nobody names keep what they held"""
    from uniir_amd import clip_front
    n = 16
    imgs, geoms = K.mixed_batch(n)
    slots = [8, 0, 5, 2, 9, 3, 6]
    plain = clip_front.PackedImages(imgs, geoms, n, out_index=slots, out_items=10)
    aug = clip_front.PackedImages(imgs, geoms, n, out_index=slots, out_items=10, augs=[[("Identity", 0.0)] * 2] * 7)
    assert plain.aug_info is None and aug.aug_info is not None and aug.aug_info.launches_preprocess == 8
    a = plain.run(DEV, out=torch.full((10, 3, n, n), -5.0, device=DEV))
    b = aug.run(DEV, out=torch.full((10, 3, n, n), -5.0, device=DEV))
    assert torch.equal(a, b)
    assert all((b[s] == -5.0).all().item() for s in (1, 4, 7)) and not (b[8] == -5.0).any().item()
    none = clip_front.PackedImages(imgs, geoms, n, out_index=slots, out_items=10, augs=[None] * 7)          # no slot at all
    assert torch.equal(none.run(DEV, out=torch.full((10, 3, n, n), -5.0, device=DEV)), a)
    for i, s in enumerate(slots):
        assert np.array_equal(a[s].cpu().numpy(), K.reference(imgs[i], geoms[i], n)), i


def test_pipeline_with_ops_equals_resize_then_restatement():
    """the _aug entry on the mixed batch with real ops: the oracle's resized bytes, the restatement's ops, ToTensor + Normalize"""
    from oracle import c_oracle
    from uniir_amd import clip_front
    n = 24
    imgs, geoms = K.mixed_batch(n)
    _, lists = _mixed(n)
    got = clip_front.PackedImages(imgs, geoms, n, augs=lists).run(DEV).cpu().numpy()
    for i, (img, g) in enumerate(zip(imgs, geoms)):
        left, top, bw, bh, oh, ow, wtop, wleft, flip = g
        r = c_oracle.resize_bicubic(img[top:top + bh, left:left + bw], oh, ow)[wtop:wtop + n, wleft:wleft + n]
        r = np.ascontiguousarray(r[:, ::-1] if flip else r)
        x = R.apply_ops(r, lists[i] or []).astype(np.float32) / np.float32(255.0)
        want = (x.transpose(2, 0, 1) - np.float32(K.MEAN)[:, None, None]) / np.float32(K.STD)[:, None, None]
        assert np.array_equal(got[i], want.astype(np.float32)), i


def test_raw_blip_transform_with_randaugment_end_to_end():
    """8 images: get_blip_transform(32, randaugment=(2, 5)) on the host == RawBlipTransform(32, randaugment=(2, 5)) ->
    RawImageBatch.to_device from the same random / np.random states, bit for bit, and the same states afterwards"""
    from PIL import Image
    from uniir_amd import blip_front, clip_front
    n = 32
    pils = [Image.fromarray(K.image(h, w, 70 + i), "RGB") for i, (w, h) in enumerate([(120, 90), (37, 53), (256, 171), (64, 64)] * 2)]
    host = blip_front.get_blip_transform(n, randaugment=(2, 5))
    raw = blip_front.RawBlipTransform(n, randaugment=(2, 5))
    random.seed(11)
    np.random.seed(3)
    want = [host(p) for p in pils]
    states = random.getstate(), np.random.get_state()
    random.seed(11)
    np.random.seed(3)
    items = [raw(p) for p in pils]
    assert random.getstate() == states[0]
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], states[1][1:3]))
    drawn = {name for it in items for name, _ in it.ops}
    assert len(drawn - {"Identity"}) >= 3, drawn
    batch = clip_front.RawImageBatch(items[:3] + [None] + items[3:], raw)
    got = batch.pin_memory().to_device(DEV)
    assert batch._packed.aug_info is not None
    assert got.shape == (9, 3, n, n) and (got[3] == 0).all().item()
    for row, w in zip((0, 1, 2, 4, 5, 6, 7, 8), want):
        assert torch.equal(got[row].cpu(), w), (row, items[row - (row > 3)].ops)
    assert torch.equal(clip_front.RawImageBatch(items[:3] + [None] + items[3:], raw).to_device(DEV), got)     # a second run


def _library_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sorted(e.name.split("(")[0].replace("void ", "") for e in prof.events()
                  if e.device_type == torch.autograd.DeviceType.CUDA and "img_" in e.name)


def test_launch_count_does_not_depend_on_the_batch_size():
    from uniir_amd import clip_front
    n = 24
    imgs, geoms = K.mixed_batch(n)
    _, lists = _mixed(n)
    seven = clip_front.PackedImages(imgs, geoms, n, augs=lists)
    one = clip_front.PackedImages(imgs[:1], geoms[:1], n, augs=lists[:1])
    assert seven.aug_info.launches_preprocess == one.aug_info.launches_preprocess == 8
    out7, out1 = torch.empty(7, 3, n, n, device=DEV), torch.empty(1, 3, n, n, device=DEV)
    b7, b1 = seven.blob.to(DEV), one.blob.to(DEV)
    first = seven.run(DEV, out=out7, blob=b7).clone()
    k7 = _library_kernels(lambda: seven.run(DEV, out=out7, blob=b7))
    k1 = _library_kernels(lambda: one.run(DEV, out=out1, blob=b1))
    print("kernels of 7 images:", k7, " of 1 image:", k1)
    assert k7 == k1
    if k7:                  # a profiler that records the library's kernels: what the plan reports is what ran
        assert len(k7) == seven.aug_info.launches_preprocess
    assert torch.equal(out7, first) and torch.equal(out1[0], out7[0])
