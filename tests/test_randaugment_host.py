"""CPU tests of the augmentation's host side, through the C ABI where there is one (no device): uniir_image_aug_plan's refusals,
table and summary; the host transform get_blip_transform(..., randaugment=(2, 5)) against the restatement applied by hand; and
that randaugment=None is today's function bit for bit."""
import ctypes
import math
import random

import numpy as np
import pytest
import torch

import image_batch_cases as K
import randaugment_ref as R


def _plan(ops, args, count, slots, n, table="auto", info="auto", raw_ops=None):
    from uniir_amd import _lib
    lib = _lib.load()
    o = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(-1))
    a = np.ascontiguousarray(np.asarray(args, dtype=np.float64).reshape(-1))
    tab = (_lib.ImageAug * max(count, 1))() if table == "auto" else table
    inf = _lib.ImageAugInfo() if info == "auto" else info
    code = lib.uniir_image_aug_plan(
        o.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if raw_ops is None else raw_ops[0],
        a.ctypes.data_as(ctypes.POINTER(ctypes.c_double)) if raw_ops is None else raw_ops[1],
        count, slots, n, tab, None if inf is None else ctypes.byref(inf))
    return code, tab, inf


def test_plan_refusals():
    """every refusal of the header's list, with its code; a good table right after, so that a refusal is not a stuck state"""
    EINVAL, EUNSUPPORTED = -1, -5
    good = ([[9, 1], [0, 3]], [[15.0, 0.0], [0.0, 1.0]])
    assert _plan(*good, 2, 2, 24)[0] == 0
    assert _plan([[11, 0]], [[0.0, 0.0]], 1, 2, 24)[0] == EINVAL                    # unknown op code
    assert _plan([[-1, 0]], [[0.0, 0.0]], 1, 2, 24)[0] == EINVAL
    for bad in (float("nan"), float("inf"), -float("inf")):                          # non-finite argument, any op
        assert _plan([[9, 0]], [[bad, 0.0]], 1, 2, 24)[0] == EINVAL
        assert _plan([[0, 0]], [[0.0, bad]], 1, 2, 24)[0] == EINVAL
    assert _plan([[0] * 5], [[0.0] * 5], 1, 5, 24)[0] == EINVAL                      # more than 4 slots
    assert _plan([[0] * 4], [[0.0] * 4], 1, 4, 24)[0] == 0
    assert _plan(*good, 2, -1, 24)[0] == EINVAL
    assert _plan(*good, 2, 2, 24, table=None)[0] == EINVAL                           # null pointers
    assert _plan(*good, 2, 2, 24, info=None)[0] == EINVAL
    assert _plan(*good, 2, 2, 24, raw_ops=(None, None))[0] == EINVAL
    assert _plan(*good, 2, 2, 0)[0] == EINVAL and _plan(*good, -1, 2, 24)[0] == EINVAL
    assert _plan(*good, 2, 2, 2049)[0] == EUNSUPPORTED
    assert _plan([[5, 0]], [[1e7, 0.0]], 1, 2, 24)[0] == EUNSUPPORTED                # the fixed-point range is no place for it
    assert _plan(*good, 2, 2, 24)[0] == 0
    code, _, info = _plan([], [], 0, 2, 24, table=None)
    assert code == 0 and info.launches == 0 and info.workspace_bytes == 0


def test_plan_table_and_summary():
    """the table holds what the restatement computes on the host, bit for bit: the fp64 inverse matrices (libm's cos / sin on
    both sides), the factors; the launch count does not depend on the batch size; the workspace is two byte buffers + the tables"""
    n = 19
    ops = [("Rotate", 15.0), ("Rotate", -15.0), ("Rotate", 180.0), ("Rotate", 33.3), ("ShearX", 0.15), ("ShearY", -0.15),
           ("TranslateX", 5.0), ("TranslateY", -5.0), ("ShearX", 0.24000000000000002), ("Brightness", 1.54), ("Sharpness", 0.64),
           ("Equalize", 0.0), ("AutoContrast", 0.0), ("AutoContrastPIL", 0.0), ("Identity", 0.0)]
    codes = [[R.CODES[name], 0] for name, _ in ops]
    args = [[arg, 0.0] for _, arg in ops]
    code, tab, info = _plan(codes, args, len(ops), 2, n)
    assert code == 0
    for i, (name, arg) in enumerate(ops):
        s = tab[i].slot[0]
        assert s.op == R.CODES[name] and tab[i].slot[1].op == 0 and tab[i].slot[3].op == 0
        if name in ("Brightness", "Sharpness"):
            assert s.p[0] == arg
        elif R.CODES[name] in range(5, 10):
            want = R.invert(R.forward_matrix(name, arg, n, n))
            assert list(s.p) == want[0] + want[1], (name, arg, list(s.p), want)
    al = lambda x: (x + 255) & ~255
    assert info.workspace_bytes == 2 * al(3 * len(ops) * n * n) + al(768 * len(ops))
    assert (info.count, info.n, info.slots, info.launches, info.launches_preprocess) == (len(ops), n, 2, 4, 8)
    one = _plan(codes[:1], args[:1], 1, 2, n)[2]
    assert (one.launches, one.launches_preprocess) == (info.launches, info.launches_preprocess)
    # the product's own host matrix is the same function
    from uniir_amd import randaugment
    for name, arg in ops[:9]:
        want = R.invert(R.forward_matrix(name, arg, n, n))
        assert list(randaugment.inverse_matrix(name, arg, n, n)) == want[0] + want[1]
    assert randaugment.OP_CODES == R.CODES and list(randaugment.AUGS) == R.AUGS


def test_product_ops_equal_the_restatement():
    """uniir_amd/randaugment.apply_ops (the shipped host path) == tests/randaugment_ref, op by op, both signs, odd and even sizes"""
    from uniir_amd import randaugment
    rng = np.random.default_rng(21)
    imgs = [rng.integers(0, 256, (n, n, 3), dtype=np.uint8) for n in (16, 19)] + list(R.lut_cases().values()) + [R.smooth_image(24)]
    ops = [("Identity", 0.0), ("AutoContrast", 0.0), ("AutoContrastPIL", 0.0), ("Equalize", 0.0), ("Brightness", 0.1), ("Brightness", 1.9),
           ("Sharpness", 1.0), ("Sharpness", 0.0), ("Sharpness", 0.64), ("Sharpness", 1.9), ("ShearX", 0.15), ("ShearX", -0.15),
           ("ShearY", 0.15), ("ShearY", -0.15), ("TranslateX", 5.0), ("TranslateX", -5.0), ("TranslateY", 5.0), ("TranslateY", -5.0),
           ("TranslateX", 2.3), ("Rotate", 15.0), ("Rotate", -15.0), ("Rotate", 180.0)]
    for img in imgs:
        for op in ops:
            assert np.array_equal(randaugment.apply_ops(img, [op]), R.apply_op(img, *op)), (img.shape, op)
    two = [("Rotate", 15.0), ("Equalize", 0.0)]
    assert np.array_equal(randaugment.apply_ops(imgs[1], two), R.apply_ops(imgs[1], two))


def test_product_draw_equals_the_restatement_draw():
    from uniir_amd import blip_front
    for M in (5, 8):
        np.random.seed(4)
        want = [R.RandAugmentDraw(2, M).draw() for _ in range(40)]
        state = np.random.get_state()
        np.random.seed(4)
        got = [blip_front.RandAugmentDraw(2, M).draw() for _ in range(40)]
        assert got == want and all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], state[1:3]))
    with pytest.raises(ValueError):
        blip_front.RandAugmentDraw(2, 5, augs=["Solarize"])
    with pytest.raises(ValueError):
        blip_front.RandAugmentDraw(5, 5)


def _pils():
    from PIL import Image
    return [Image.fromarray(K.image(h, w, 60 + i), "RGB") for i, (w, h) in enumerate([(120, 90), (37, 53), (64, 64), (99, 41)] * 3)]


def test_host_transform_with_randaugment_equals_the_restatement_by_hand():
    """seeded `random` (box, flip) and np.random (ops): train_fn's tensor == box / resize / flip by hand with Pillow, the drawn ops
    by the restatement, ToTensor + Normalize; the same states afterwards; the twelve images draw real work"""
    from PIL import Image
    from uniir_amd import blip_front
    n = 32
    host = blip_front.get_blip_transform(n, is_train=True, randaugment=(2, 5))
    pils = _pils()
    random.seed(7)
    np.random.seed(3)
    got = [host(p) for p in pils]
    states = random.getstate(), np.random.get_state()
    random.seed(7)
    np.random.seed(3)
    draw, used = R.RandAugmentDraw(2, 5), set()
    for p, g in zip(pils, got):
        (left, top, bw, bh, flip), _ = K.blip_train_draws(*p.size)
        im = p.crop((left, top, left + bw, top + bh)).resize((n, n), Image.BICUBIC)
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        ops = draw.draw()
        used.update(name for name, _ in ops)
        a = R.apply_ops(np.array(im), ops).astype(np.float32) / np.float32(255.0)
        want = (a.transpose(2, 0, 1) - np.float32(K.MEAN)[:, None, None]) / np.float32(K.STD)[:, None, None]
        assert g.dtype == torch.float32 and np.array_equal(g.numpy(), want.astype(np.float32)), ops
    assert random.getstate() == states[0]
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], states[1][1:3]))
    assert len(used - {"Identity"}) >= 4, used


def test_randaugment_none_is_todays_transform():
    """no keyword, None, and eval mode with the keyword: the tensors of the transform as it was, and np.random untouched"""
    from PIL import Image
    from uniir_amd import blip_front
    n = 24
    pils = _pils()[:4]
    np.random.seed(1)
    before = np.random.get_state()
    for is_train in (True, False):
        outs = []
        for kw in ({}, {"randaugment": None}):
            random.seed(13)
            outs.append([blip_front.get_blip_transform(n, is_train=is_train, **kw)(p) for p in pils])
        assert all(torch.equal(a, b) for a, b in zip(*outs))
        random.seed(13)             # the transform as it was, by hand
        for p, g in zip(pils, outs[0]):
            if is_train:
                (left, top, bw, bh, flip), _ = K.blip_train_draws(*p.size)
                im = p.crop((left, top, left + bw, top + bh)).resize((n, n), Image.BICUBIC)
                im = im.transpose(Image.FLIP_LEFT_RIGHT) if flip else im
            else:
                im = p.resize((n, n), Image.BICUBIC)
            a = np.asarray(im, dtype=np.float32) / np.float32(255.0)
            want = (a.transpose(2, 0, 1) - np.float32(K.MEAN)[:, None, None]) / np.float32(K.STD)[:, None, None]
            assert np.array_equal(g.numpy(), want.astype(np.float32))
    random.seed(13)
    ev = [blip_front.get_blip_transform(n, is_train=False, randaugment=(2, 5))(p) for p in pils]      # eval never augments
    random.seed(13)
    assert all(torch.equal(a, b) for a, b in zip(ev, [blip_front.get_blip_transform(n, is_train=False)(p) for p in pils]))
    assert all(np.array_equal(a, b) for a, b in zip(np.random.get_state()[1:3], before[1:3]))


def test_raw_transform_carries_the_drawn_ops_and_packs_the_table():
    """RawBlipTransform(randaugment=(2, 5)) draws box, flip (random) and ops (np.random) as the host transform does and carries
    them on the RawImage; PackedImages puts the aug table of the plan call into the one buffer, between the plan table and the
    pixels; an all-Identity batch packs no table (the plain entry point: same bits); model surface passes the keyword on"""
    from types import SimpleNamespace
    from uniir_amd import _lib, blip_front, blip_model, clip_front
    n = 32
    raw = blip_front.RawBlipTransform(n, is_train=True, randaugment=(2, 5))
    pils = _pils()[:6]
    random.seed(7)
    np.random.seed(3)
    items = [raw(p) for p in pils]
    random.seed(7)
    np.random.seed(3)
    draw = R.RandAugmentDraw(2, 5)
    for p, it in zip(pils, items):
        geom, _ = K.blip_train_draws(*p.size)
        assert it.geom == geom and it.ops == draw.draw()
    assert blip_front.RawBlipTransform(n, is_train=False, randaugment=(2, 5))(pils[0]).ops is None
    assert blip_front.RawBlipTransform(n, is_train=True)(pils[0]).ops is None
    packed = clip_front.RawImageBatch([items[0], None] + items[1:], raw)._pack(pin=False)
    assert packed.aug_info is not None and packed.aug_info.slots == 2 and packed.aug_info.count == 6
    na = 6 * ctypes.sizeof(_lib.ImageAug)
    assert packed.plan0 < packed.aug0 < packed.pix0 and packed.pix0 - packed.aug0 == (na + 255) & ~255
    tab = (_lib.ImageAug * 6).from_buffer_copy(packed.blob.numpy()[packed.aug0:packed.aug0 + na].tobytes())
    for i, it in enumerate(items):
        assert [tab[i].slot[k].op for k in range(2)] == [R.CODES[name] for name, _ in it.ops]
    a = packed.blob.numpy()
    d0 = packed.descs[0]
    assert np.array_equal(a[packed.pix0 + d0.offset:packed.pix0 + d0.offset + items[0].data.numel()], items[0].data.numpy().reshape(-1))
    idle = [clip_front.RawImage(it.data, it.geom, [("Identity", 0.0)] * 2) for it in items]
    assert clip_front.RawImageBatch(idle, raw)._pack(pin=False).aug_info is None
    assert clip_front.RawImageBatch([clip_front.RawImage(it.data, it.geom) for it in items], raw)._pack(pin=False).aug_info is None
    model = SimpleNamespace(image_size=n, training=True)
    fn = blip_model.BLIPFeatureFusion.get_img_preprocess_fn(model, raw=True, randaugment=(2, 5))
    assert isinstance(fn, blip_front.RawBlipTransform) and (fn.randaugment.N, fn.randaugment.M) == (2, 5)
    assert blip_model.BLIPScoreFusion.get_img_preprocess_fn is blip_model.BLIPFeatureFusion.get_img_preprocess_fn
    assert math.isclose(fn.randaugment.M / 10 * 30, 15.0)
