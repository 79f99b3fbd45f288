"""CPU tests of the batched device image transform's host side: blip_front.RawBlipTransform draws what get_blip_transform's
train_fn draws (same calls, order and count of `random`), and uniir_image_batch_plan -- pure host arithmetic -- lays the
workspace out as an independent restatement does and rejects every malformed descriptor table with its code."""
import ctypes
import random

import numpy as np
import pytest

import image_batch_cases as K

SIZES = [(500, 375), (375, 500), (64, 64), (33, 200), (10, 400), (400, 10)]       # (w, h); the last two only fit the fallback box


def test_raw_blip_transform_draws_what_train_fn_draws():
    from uniir_amd.blip_front import RawBlipTransform
    tf = RawBlipTransform(24, min_scale=0.5, is_train=True)
    fallbacks = {s: 0 for s in SIZES}
    for seed in range(200):
        for w, h in SIZES:
            random.seed(seed)
            want, fb = K.blip_train_draws(w, h)
            state = random.getstate()
            random.seed(seed)
            got = tf.draw(w, h)
            assert got == want, (seed, w, h, got, want)
            assert random.getstate() == state, (seed, w, h)
            left, top, bw, bh, flip = got
            assert 0 <= left and 0 <= top and bw > 0 and bh > 0 and left + bw <= w and top + bh <= h and flip in (0, 1)
            fallbacks[(w, h)] += fb
    assert fallbacks[(10, 400)] == fallbacks[(400, 10)] == 200 and fallbacks[(500, 375)] == 0, fallbacks
    ev = RawBlipTransform(24, is_train=False)
    assert ev.is_train is False and ev.n_px == 24 and ev.center_crop is False


def test_raw_blip_transform_by_hand_with_pillow_equals_train_fn():
    """decode + draw in RawBlipTransform, then box / resize / flip applied by hand with Pillow == train_fn's tensor, and the
    `random` state afterwards is the same; eval mode draws nothing"""
    Image = pytest.importorskip("PIL.Image")
    import torch
    from uniir_amd import blip_front
    n = 24
    host, raw = blip_front.get_blip_transform(n, is_train=True), blip_front.RawBlipTransform(n, is_train=True)
    for seed, (w, h) in enumerate(SIZES + [(37, 53), (7, 5)]):
        pil = Image.fromarray(K.image(h, w, seed), "RGB")
        random.seed(1000 + seed)
        want = host(pil)
        state = random.getstate()
        random.seed(1000 + seed)
        item = raw(pil)
        assert random.getstate() == state
        assert item.data.dtype == torch.uint8 and tuple(item.data.shape) == (h, w, 3)
        left, top, bw, bh, flip = item.geom
        im = Image.fromarray(item.data.numpy(), "RGB").crop((left, top, left + bw, top + bh)).resize((n, n), Image.BICUBIC)
        if flip:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        assert torch.equal(blip_front._to_tensor_normalized(im), want), (w, h)
        assert np.array_equal(K.reference_pil(item.data.numpy(), (left, top, bw, bh, n, n, 0, 0, flip), n), want.numpy())
    state = random.getstate()
    item = blip_front.RawBlipTransform(n, is_train=False)(pil)
    assert item.geom is None and random.getstate() == state


def _lib():
    from uniir_amd import _lib
    return _lib, _lib.load()


def _table(geoms, sizes, out_index=None):
    """descriptor table of images packed back to back at 16-byte aligned offsets -> (ctypes array, packed bytes)"""
    L, _ = _lib()
    descs, off = (L.ImageDesc * len(geoms))(), 0
    for i, (g, (w, h)) in enumerate(zip(geoms, sizes)):
        d = descs[i]
        d.offset, d.h, d.w = off, h, w
        d.box_left, d.box_top, d.box_w, d.box_h, d.oh, d.ow, d.top, d.left, d.flip = g
        d.out_index = i if out_index is None else out_index[i]
        off += (3 * h * w + 15) & ~15
    return descs, off


def _plan(descs, count, n, out_items, packed):
    L, lib = _lib()
    plans, info = (L.ImagePlan * max(count, 1))(), L.ImageBatchInfo()
    return lib.uniir_image_batch_plan(descs, count, n, out_items, packed, plans, ctypes.byref(info)), plans, info


def _check_against_restatement(geoms, sizes, n):
    descs, packed = _table(geoms, sizes)
    code, plans, info = _plan(descs, len(geoms), n, len(geoms), packed)
    assert code == 0
    want, ws, max_rows = K.expected_plan(geoms, n)
    assert (info.workspace_bytes, info.max_rows, info.count, info.n, info.out_items) == (ws, max_rows, len(geoms), n, len(geoms))
    for i, w in enumerate(want):
        got = {k: getattr(plans[i], k) for k in w}
        assert got == w, (i, geoms[i], got, w)
        bh, top = geoms[i][3], geoms[i][6]
        assert 0 <= w["y0"] and w["y0"] + w["rows"] <= bh and 0 <= w["x0"] and w["x0"] + w["cols"] <= geoms[i][2]
    return info


def test_plan_equals_the_restated_bound_arithmetic():
    launches = set()
    for n in (16, 24, 32):
        _, geoms = K.mixed_batch(n)
        launches.add(_check_against_restatement(geoms, K.MIXED_SIZES, n).launches)
    for box, n in K.BOX_CASES:
        _, geoms = K.box_batch(box, n)
        launches.add(_check_against_restatement(geoms, [(80, 64)] * 2, n).launches)
    launches.add(_check_against_restatement([K.clip_geom(375, 500, 224)], [(500, 375)], 224).launches)
    assert len(launches) == 1 and launches.pop() > 0            # the same number of launches whatever the batch
    # the skipped passes: no table, the rows / columns of the window itself
    descs, packed = _table([(3, 5, 16, 40, 16, 16, 0, 0, 0)], [(80, 64)])
    _, plans, _ = _plan(descs, 1, 16, 1, packed)
    assert (plans[0].kx, plans[0].x0, plans[0].cols) == (0, 0, 16) and plans[0].ky > 0
    # count == 0: valid, nothing to do
    code, _, info = _plan(None, 0, 16, 4, 0)
    assert code == 0 and info.workspace_bytes == 0 and info.count == 0 and info.launches == 0


_OK = dict(geom=(4, 6, 40, 30, 20, 24, 2, 3, 1), size=(80, 64), n=16, out_items=3, out_index=1)
EINVAL, ESHAPE = -1, -2
_REJECTS = [
    ("h = 0", dict(h=0), EINVAL), ("w < 0", dict(w=-3), EINVAL), ("box_w = 0", dict(box_w=0), EINVAL),
    ("box_h < 0", dict(box_h=-1), EINVAL), ("oh = 0", dict(oh=0), EINVAL), ("ow = 0", dict(ow=0), EINVAL),
    ("flip = 2", dict(flip=2), EINVAL), ("offset not 16-byte aligned", dict(offset=8), EINVAL),
    ("out_index = out_items", dict(out_index=3), EINVAL), ("out_index < 0", dict(out_index=-1), EINVAL),
    ("box past the right edge", dict(box_left=41), ESHAPE), ("box past the bottom", dict(box_top=35), ESHAPE),
    ("box_left < 0", dict(box_left=-1), ESHAPE), ("box_top < 0", dict(box_top=-1), ESHAPE),
    ("window past ow", dict(left=9), ESHAPE), ("window past oh", dict(top=5), ESHAPE),
    ("window left < 0", dict(left=-1), ESHAPE), ("window top < 0", dict(top=-1), ESHAPE),
    ("image past the packed buffer", dict(offset=16), ESHAPE),
]


def test_plan_rejects_every_malformed_table_on_the_host():
    L, lib = _lib()
    descs, packed = _table([_OK["geom"]], [_OK["size"]], [_OK["out_index"]])
    assert _plan(descs, 1, _OK["n"], _OK["out_items"], packed)[0] == 0
    wrong = []
    for what, changes, want in _REJECTS:
        descs, packed = _table([_OK["geom"]], [_OK["size"]], [_OK["out_index"]])
        for k, v in changes.items():
            setattr(descs[0], k, v)
        got = _plan(descs, 1, _OK["n"], _OK["out_items"], packed)[0]
        if got != want:
            wrong.append((what, got, want))
    assert not wrong, wrong
    descs, packed = _table([_OK["geom"]] * 2, [_OK["size"]] * 2, [2, 2])                 # two descriptors, one slot
    assert _plan(descs, 2, 16, 3, packed)[0] == EINVAL
    descs, packed = _table([_OK["geom"]] * 2, [_OK["size"]] * 2, [2, 0])
    assert _plan(descs, 2, 16, 3, packed)[0] == 0
    assert _plan(descs, 2, 16, 3, packed - 16)[0] == ESHAPE                              # the last image ends past the buffer
    plans, info = (L.ImagePlan * 2)(), L.ImageBatchInfo()
    assert lib.uniir_image_batch_plan(None, 2, 16, 3, packed, plans, ctypes.byref(info)) == EINVAL
    assert lib.uniir_image_batch_plan(descs, 2, 16, 3, packed, None, ctypes.byref(info)) == EINVAL
    assert lib.uniir_image_batch_plan(descs, 2, 16, 3, packed, plans, None) == EINVAL
    for count, n, out_items in ((-1, 16, 3), (2, 0, 3), (2, -4, 3), (2, 16, 0)):
        assert lib.uniir_image_batch_plan(descs, count, n, out_items, packed, plans, ctypes.byref(info)) == EINVAL
    # the launch call checks its own arguments before anything else: no device is needed to be turned away
    _, _, info = _plan(descs, 2, 16, 3, packed)
    m = (ctypes.c_float * 3)(*K.MEAN)
    assert info.workspace_bytes > 0
    assert lib.uniir_image_preprocess_batch(0x10000, 0x20000, 0x30000, None, m, m, 0x40000, 0x50000, 1 << 30, None) == EINVAL
    for args in ((None, 0x20000, 0x30000, 0x40000, 0x50000, 1 << 30), (0x10000, None, 0x30000, 0x40000, 0x50000, 1 << 30),
                 (0x10000, 0x20000, None, 0x40000, 0x50000, 1 << 30), (0x10000, 0x20000, 0x30000, None, 0x50000, 1 << 30),
                 (0x10000, 0x20000, 0x30000, 0x40000, None, 1 << 30),
                 (0x10000, 0x20000, 0x30000, 0x40000, 0x50000, info.workspace_bytes - 1),          # workspace too small
                 (0x10000, 0x20000, 0x30000, 0x40000, 0x50010, 1 << 30)):                           # workspace misaligned
        px, de, pl, out, ws, wsb = args
        assert lib.uniir_image_preprocess_batch(px, de, pl, ctypes.byref(info), m, m, out, ws, wsb, None) == EINVAL, args
    assert lib.uniir_image_preprocess_batch(0x10000, 0x20000, 0x30000, ctypes.byref(info), None, m, 0x40000, 0x50000, 1 << 30,
                                            None) == EINVAL


def test_packed_images_layout_and_host_validation():
    """clip_front.PackedImages: [descriptor table | plan table | pixels] in one buffer, images at 16-byte aligned offsets;
    a malformed geometry raises on the host"""
    from uniir_amd import _lib, clip_front
    imgs, geoms = K.mixed_batch(16)
    p = clip_front.PackedImages(imgs, geoms, 16, out_index=[6, 0, 3, 1, 5, 2, 4], out_items=8)
    assert p.count == 7 and p.out_items == 8 and p.plan0 % 256 == 0 and p.pix0 % 256 == 0
    blob = p.blob.numpy()
    assert bytes(blob[:7 * ctypes.sizeof(_lib.ImageDesc)]) == bytes(p.descs)[:7 * ctypes.sizeof(_lib.ImageDesc)]
    assert bytes(blob[p.plan0:p.plan0 + 7 * ctypes.sizeof(_lib.ImagePlan)]) == bytes(p.plans)
    for i, a in enumerate(imgs):
        off = p.descs[i].offset
        assert off % 16 == 0 and np.array_equal(blob[p.pix0 + off:p.pix0 + off + a.size], a.reshape(-1))
    assert p.info.workspace_bytes == K.expected_plan(geoms, 16)[1]
    whole = clip_front.PackedImages(imgs[:1], None, 16)                   # None = the CLIP chain on the whole image
    d = whole.descs[0]
    assert (d.box_left, d.box_top, d.box_w, d.box_h, d.oh, d.ow, d.top, d.left, d.flip) == K.clip_geom(53, 37, 16)
    with pytest.raises(RuntimeError):
        clip_front.PackedImages(imgs[:1], [(0, 0, 38, 53, 16, 16, 0, 0, 0)], 16)         # box wider than the image
    with pytest.raises(RuntimeError):
        clip_front.PackedImages(imgs[:2], None, 16, out_index=[1, 1])
    with pytest.raises(ValueError):
        clip_front.PackedImages([imgs[0][:, :, :2]], None, 16)
    assert clip_front.PackedImages([], None, 16, out_items=4).count == 0
