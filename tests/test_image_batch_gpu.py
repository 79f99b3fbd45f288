"""The batched device image transform (uniir_image_batch_plan + uniir_image_preprocess_batch, clip_front.PackedImages /
preprocess_batch_on_device / RawImageBatch, blip_front.RawBlipTransform) on the GPU.  Every comparison is np.array_equal: the
integer stage is Pillow's 8-bit resample bit for bit, the float stage two correctly rounded divisions.

The reference of a descriptor is four steps on the CPU (tests/image_batch_cases.reference): c_oracle.resize_bicubic of the cut
box (pinned to Pillow by G14), the window, the mirror, (x / 255 - mean) / std in fp32 -- and, where PIL imports, Pillow's own
Image.crop(box).resize() as well."""
import ctypes
import os
import random
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import image_batch_cases as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "uniir_amd", "src")
for p in (ROOT, SRC, os.path.join(SRC, "common")):
    if p not in sys.path:
        sys.path.insert(0, p)

try:
    from PIL import Image
except ImportError:          # the oracle reference alone then
    Image = None


def _check(imgs, geoms, n, got, slots=None):
    for i, (img, g) in enumerate(zip(imgs, geoms)):
        row = got[i if slots is None else slots[i]]
        want = K.reference(img, g, n)
        assert np.array_equal(row, want), (i, g, float(np.abs(row - want).max()))
        if Image is not None:
            assert np.array_equal(row, K.reference_pil(img, g, n)), (i, g)


@pytest.mark.parametrize("n", [16, 24, 32])
def test_mixed_batch_of_seven_sizes(n):
    """seven images of different sizes in one call: up- and downscaling per axis, whole-image and boxed descriptors, a window
    inside a larger resized box, flipped and unflipped; images with fewer touched rows than the largest leave the grid early"""
    from uniir_amd import clip_front
    imgs, geoms = K.mixed_batch(n)
    got = clip_front.preprocess_batch_on_device(imgs, geoms, n, DEV).cpu().numpy()
    assert got.shape == (7, 3, n, n)
    _check(imgs, geoms, n, got)


@pytest.mark.parametrize("box,n", K.BOX_CASES, ids=[f"box{b[0]}_{b[1]}_{b[2]}x{b[3]}_n{n}" for b, n in K.BOX_CASES])
def test_skipped_passes_and_extreme_boxes(box, n):
    """box_w == n takes the column copy, box_h == n the direct vertical read, both the plain cut; one pixel, one and two
    columns, a box at the right edge, the whole image -- each unflipped and flipped.  The windows are clamped at the box."""
    from uniir_amd import clip_front
    imgs, geoms = K.box_batch(box, n)
    got = clip_front.preprocess_batch_on_device(imgs, geoms, n, DEV).cpu().numpy()
    _check(imgs, geoms, n, got)
    assert np.array_equal(got[1], got[0][:, :, ::-1])


def test_clip_geometry_equals_the_per_image_entry_point():
    """G14's images: the batched output is bitwise preprocess_on_device's on the same list, centre crop and center_crop=False"""
    from uniir_amd import clip_front
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "g14_image.npz"))
    imgs = [z[f"c{c}_img"] for c in range(int(z["n_cases"]))]
    for n in sorted({int(z[f"c{c}_geom"][0]) for c in range(len(imgs))} | {32}):
        for center_crop in (True, False):
            want = clip_front.preprocess_on_device(imgs, n, DEV, center_crop=center_crop)
            geoms = [K.clip_geom(a.shape[0], a.shape[1], n, center_crop) for a in imgs]
            got = clip_front.preprocess_batch_on_device(imgs, geoms, n, DEV)
            assert torch.equal(got, want), (n, center_crop)
            if center_crop:
                assert torch.equal(clip_front.preprocess_batch_on_device(imgs, None, n, DEV), want)


def test_scatter_leaves_unnamed_slots_and_the_guard_untouched():
    from uniir_amd import clip_front
    n = 16
    imgs, geoms = K.mixed_batch(n)
    imgs, geoms, slots = imgs[:3], geoms[:3], [4, 0, 3]
    buf = torch.full((8 * 3 * n * n,), -777.0, device=DEV)
    out = buf[:6 * 3 * n * n].view(6, 3, n, n)
    res = clip_front.preprocess_batch_on_device(imgs, geoms, n, DEV, out=out, out_index=slots)
    assert res.data_ptr() == out.data_ptr()
    got = buf.cpu().numpy()
    _check(imgs, geoms, n, got[:6 * 3 * n * n].reshape(6, 3, n, n), slots)
    for s in (1, 2, 5):
        assert (got[s * 3 * n * n:(s + 1) * 3 * n * n] == -777.0).all(), s
    assert (got[6 * 3 * n * n:] == -777.0).all()


def test_one_image_and_no_image():
    from uniir_amd import clip_front
    n = 24
    imgs, geoms = K.mixed_batch(n)
    got = clip_front.preprocess_batch_on_device(imgs[3:4], geoms[3:4], n, DEV).cpu().numpy()
    _check(imgs[3:4], geoms[3:4], n, got)
    out = torch.full((2, 3, n, n), 5.0, device=DEV)
    res = clip_front.preprocess_batch_on_device([], [], n, DEV, out=out)
    assert res is out and (out == 5.0).all().item()
    # count == 0 at the C entry point: UNIIR_OK without a launch, whatever the other arguments
    from uniir_amd import _lib
    lib, info = _lib.load(), _lib.ImageBatchInfo()
    assert lib.uniir_image_batch_plan(None, 0, n, 2, 0, None, ctypes.byref(info)) == 0 and info.launches == 0
    assert lib.uniir_image_preprocess_batch(None, None, None, ctypes.byref(info), None, None, None, None, 0, None) == 0
    torch.cuda.synchronize()
    assert (out == 5.0).all().item()


_GOOD = (4, 6, 40, 30, 20, 24, 2, 3, 1)          # on an 80 x 64 image, n = 16
_BAD = [  # (what, geometry / slot changes, code)
    ("h = 0", dict(h=0), -1), ("box_w = 0", dict(box_w=0), -1), ("ow < 0", dict(ow=-2), -1),
    ("out_index = out_items", dict(out_index=3), -1), ("out_index < 0", dict(out_index=-1), -1),
    ("box past the right edge", dict(box_left=41), -2), ("box past the bottom", dict(box_top=35), -2),
    ("window past ow", dict(left=9), -2), ("window past oh", dict(top=5), -2),
    ("image past the packed buffer", dict(offset=16), -2),
]


def test_argument_errors_are_codes_and_launch_nothing():
    """one table per error of the header's list: the plan call returns its code from the host table, the Python layer raises
    before anything is copied or launched, `out` keeps its sentinel; the launch call turns away a null pointer, a short or
    misaligned workspace without a launch"""
    from uniir_amd import _lib, clip_front
    lib = _lib.load()
    n, img = 16, K.image(64, 80, 3)
    out = torch.full((3, 3, n, n), 9.0, device=DEV)

    def table(count=1, slots=(1,)):
        descs = (_lib.ImageDesc * count)()
        for i in range(count):
            d = descs[i]
            d.offset, d.h, d.w, d.out_index = i * 15360, 64, 80, slots[i]
            d.box_left, d.box_top, d.box_w, d.box_h, d.oh, d.ow, d.top, d.left, d.flip = _GOOD
        return descs

    def plan(descs, count, packed):
        plans, info = (_lib.ImagePlan * count)(), _lib.ImageBatchInfo()
        return lib.uniir_image_batch_plan(descs, count, n, 3, packed, plans, ctypes.byref(info)), plans, info

    wrong = []
    for what, changes, want in _BAD:
        descs = table()
        for k, v in changes.items():
            setattr(descs[0], k, v)
        code = plan(descs, 1, 15360)[0]
        if code != want:
            wrong.append((what, code, want))
    assert not wrong, wrong
    assert plan(table(2, (2, 2)), 2, 30720)[0] == -1                         # two descriptors, one slot
    # through the Python layer: the plan call refuses, nothing reaches the device
    for geom, slots in (((0, 0, 81, 64, n, n, 0, 0, 0), [0]), ((0, 0, 80, 64, n, n, 1, 0, 0), [0]), (_GOOD, [3]), (_GOOD, [-1])):
        with pytest.raises(RuntimeError):
            clip_front.preprocess_batch_on_device([img], [geom], n, DEV, out=out, out_index=slots)
    with pytest.raises(RuntimeError):
        clip_front.preprocess_batch_on_device([img, img], [_GOOD, _GOOD], n, DEV, out=out, out_index=[2, 2])
    # the launch call with a valid plan and real device buffers: its own checks
    packed = clip_front.PackedImages([img], [_GOOD], n, out_index=[1], out_items=3)
    blob = packed.blob.to(DEV)
    ws = torch.empty(int(packed.info.workspace_bytes) + 512, device=DEV, dtype=torch.uint8)
    m, s = (ctypes.c_float * 3)(*K.MEAN), (ctypes.c_float * 3)(*K.STD)
    base, info = blob.data_ptr(), ctypes.byref(packed.info)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    good = (base + packed.pix0, base, base + packed.plan0, info, m, s, out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
    for pos, val in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (6, None), (7, None),
                     (8, int(packed.info.workspace_bytes) - 1), (7, ws.data_ptr() + 16)):
        args = list(good)
        args[pos] = val
        assert lib.uniir_image_preprocess_batch(*args) == -1, pos
    torch.cuda.synchronize()
    assert (out == 9.0).all().item()
    assert lib.uniir_image_preprocess_batch(*good) == 0                       # ... and the untouched arguments do run
    got = out.cpu().numpy()
    assert np.array_equal(got[1], K.reference(img, _GOOD, n)) and (got[0] == 9.0).all() and (got[2] == 9.0).all()


@pytest.mark.parametrize("is_train", [True, False])
def test_raw_blip_transform_end_to_end(is_train):
    """seeded get_blip_transform on three PIL images == reseeded RawBlipTransform -> RawImageBatch (a None item in the middle)
    -> pin_memory().to_device(): rows bitwise equal, the None row zeros, the same `random` state afterwards"""
    from PIL import Image          # the host transform under comparison is Pillow's
    from uniir_amd import blip_front, clip_front
    n = 24
    pils = [Image.fromarray(K.image(h, w, 40 + i), "RGB") for i, (w, h) in enumerate([(120, 90), (37, 53), (256, 171)])]
    host, raw = blip_front.get_blip_transform(n, is_train=is_train), blip_front.RawBlipTransform(n, is_train=is_train)
    random.seed(11)
    want = [host(p) for p in pils]
    state = random.getstate()
    random.seed(11)
    items = [raw(p) for p in pils]
    assert random.getstate() == state
    batch = clip_front.RawImageBatch([items[0], None, items[1], items[2]], raw)
    assert batch.size(0) == 4 and batch.size(2) == n
    got = batch.pin_memory().to_device(DEV)
    assert got.shape == (4, 3, n, n) and got.dtype == torch.float32
    assert (got[1] == 0).all().item()
    for row, w in zip((0, 2, 3), want):
        assert torch.equal(got[row].cpu(), w), row
    assert torch.equal(clip_front.RawImageBatch([items[0], None, items[1], items[2]], raw).to_device(DEV), got)    # unpinned
    if is_train:
        assert any(it.geom[:4] != (0, 0, p.size[0], p.size[1]) for it, p in zip(items, pils))


def test_blip_model_opts_in_with_raw_and_the_collator_carries_the_geometry(tmp_path):
    """BLIP's get_img_preprocess_fn(raw=True) through dataset -> collator -> DevicePrefetcher: for a seeded loader the image
    tensor is bitwise the host transform's (train mode: random boxes and flips), image-less items stay black"""
    from data.mbeir_dataset import MBEIRCandidatePoolCollator, MBEIRCandidatePoolDataset
    from test_pipeline_gpu import _make_tree, _toy_tokenize
    from uniir_amd import blip_front, blip_model
    from uniir_amd.host_utils import DevicePrefetcher
    root = str(tmp_path)
    _make_tree(root, n_cand=9, n_query=3)
    pool = os.path.join("cand_pool", "mbeir_toy_cand_pool.jsonl")
    n = 24
    model = SimpleNamespace(image_size=n, training=True)
    fns = {"cpu": blip_model.BLIPFeatureFusion.get_img_preprocess_fn(model),
           "gpu": blip_model.BLIPFeatureFusion.get_img_preprocess_fn(model, raw=True)}
    assert isinstance(fns["gpu"], blip_front.RawBlipTransform) and fns["gpu"].is_train and not callable(getattr(fns["cpu"], "draw", None))
    batches = {}
    for mode, fn in fns.items():
        ds = MBEIRCandidatePoolDataset(root, pool, fn, print_config=False)
        col = MBEIRCandidatePoolCollator(tokenizer=_toy_tokenize, image_size=(n, n))
        if mode == "gpu":
            col.raw_transform = fn
        random.seed(5)
        batch = col([ds[i] for i in range(len(ds))])
        batches[mode] = next(iter(DevicePrefetcher([batch], 0)))
    a, b = batches["cpu"]["image_batched"], batches["gpu"]["image_batched"]
    assert a.is_cuda and b.is_cuda and a.shape == b.shape == (9, 3, n, n)
    assert torch.equal(a, b)
    mask = batches["gpu"]["image_mask_batched"]
    assert (b[mask == 0] == 0).all() and mask.sum().item() == 6


def _library_kernels(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sorted(e.name.split("(")[0].replace("void ", "") for e in prof.events()
                  if e.device_type == torch.autograd.DeviceType.CUDA and "img_" in e.name)


def test_launch_count_does_not_depend_on_the_batch_size():
    """the kernels of one batched call of 7 images and of 1 image, as the plan reports them and as the profiler sees them"""
    from uniir_amd import clip_front
    n = 16
    imgs, geoms = K.mixed_batch(n)
    seven, one = clip_front.PackedImages(imgs, geoms, n), clip_front.PackedImages(imgs[:1], geoms[:1], n)
    assert seven.info.launches == one.info.launches > 0
    out7, out1 = torch.empty(7, 3, n, n, device=DEV), torch.empty(1, 3, n, n, device=DEV)
    b7, b1 = seven.blob.to(DEV), one.blob.to(DEV)
    seven.run(DEV, out=out7, blob=b7)                    # once outside the profiler: module load, allocator
    k7 = _library_kernels(lambda: seven.run(DEV, out=out7, blob=b7))
    k1 = _library_kernels(lambda: one.run(DEV, out=out1, blob=b1))
    print("kernels of 7 images:", k7, " of 1 image:", k1)
    assert k7 == k1
    if k7:                  # a profiler that records the library's kernels: what the plan reports is what ran
        assert len(k7) == seven.info.launches
        per_image = _library_kernels(lambda: clip_front.preprocess_on_device(imgs, n, DEV))
        assert len(per_image) > len(k7)
    _check(imgs, geoms, n, out7.cpu().numpy())
