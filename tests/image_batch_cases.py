"""Cases and CPU references shared by tests/test_image_batch_gpu.py and tests/test_image_batch_host.py: descriptor tables of
the batched device image transform (include/uniir_hip.h [IMAGE]: uniir_image_batch_plan / uniir_image_preprocess_batch).

A geometry is the 9-tuple clip_front.PackedImages takes: (box_left, box_top, box_w, box_h, oh, ow, top, left, flip)."""
import math

import numpy as np

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)

# (w, h) of the seven images of the mixed batch
MIXED_SIZES = [(37, 53), (64, 48), (19, 19), (120, 90), (33, 200), (7, 5), (256, 171)]
# boxes (left, top, w, h) on a 64 (rows) x 80 (columns) image, with the n they run at: one axis unchanged (the skipped passes),
# both unchanged, one pixel, one column, two columns, the right edge, the whole image
BOX_CASES = [((3, 5, 16, 40), 16), ((3, 5, 40, 16), 16), ((10, 10, 16, 16), 16), ((79, 63, 1, 1), 16), ((0, 0, 1, 64), 16),
             ((0, 40, 2, 24), 24), ((64, 0, 16, 64), 32), ((0, 0, 80, 64), 16)]


def image(h, w, seed):
    """random bytes with saturated patches, so that the clip to [0, 255] of both passes is exercised"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[: max(h // 3, 1), : max(w // 3, 1)] = rng.choice(np.array([0, 255], dtype=np.uint8), (max(h // 3, 1), max(w // 3, 1), 3))
    return a


def clip_geom(h, w, n, center_crop=True):
    """torchvision Resize(n) + CenterCrop(n) on the whole image (clip_front.resize_geometry), or the square Resize((n, n))"""
    if not center_crop:
        return (0, 0, w, h, n, n, 0, 0, 0)
    if w <= h:
        ow, oh = n, int(n * h / w)
    else:
        oh, ow = n, int(n * w / h)
    return (0, 0, w, h, oh, ow, int(round((oh - n) / 2.0)), int(round((ow - n) / 2.0)), 0)


def mixed_batch(n):
    """the seven images with their geometries at window size n: whole-image CLIP chains (some axes up-, some downscaled), boxed
    BLIP-style descriptors (box -> n x n), a box resized to a larger size with an off-centre window; flipped and unflipped"""
    imgs = [image(h, w, 100 + i) for i, (w, h) in enumerate(MIXED_SIZES)]
    geoms = [
        clip_geom(53, 37, n),                                  # whole image, centre crop, mostly downscaling
        (5, 7, 50, 30, n, n, 0, 0, 1),                         # box -> n x n, flipped
        (0, 0, 19, 19, n, n, 0, 0, 1),                         # whole image -> n x n (19 -> 16: down; 19 -> 24 / 32: up), flipped
        (10, 20, 100, 60, n + 9, n + 5, 4, 3, 0),              # box -> (n + 9) x (n + 5), window at (4, 3)
        clip_geom(200, 33, n)[:8] + (1,),                      # tall image: the centre crop sits far down the resized image, flipped
        (1, 0, 5, 5, n, n, 0, 0, 0),                           # tiny box, heavy upscaling on both axes
        (17, 3, 200, 160, n, n, 0, 0, 0),                      # large box, heavy downscaling
    ]
    return imgs, geoms


def box_batch(box, n, seed=7):
    """the 64 x 80 image with one box, unflipped and flipped -> (images, geometries)"""
    img = image(64, 80, seed)
    left, top, bw, bh = box
    return [img, img], [(left, top, bw, bh, n, n, 0, 0, 0), (left, top, bw, bh, n, n, 0, 0, 1)]


def reference(img, geom, n, mean=MEAN, std=STD):
    """the issue's four steps on the CPU: oracle resize of the cut box, the window, the mirror, (x / 255 - mean) / std in fp32"""
    from oracle import c_oracle
    left, top, bw, bh, oh, ow, wtop, wleft, flip = geom
    r = c_oracle.resize_bicubic(img[top:top + bh, left:left + bw], oh, ow)[wtop:wtop + n, wleft:wleft + n]
    if flip:
        r = r[:, ::-1]
    x = r.astype(np.float32) / np.float32(255.0)
    return ((x.transpose(2, 0, 1) - np.float32(mean)[:, None, None]) / np.float32(std)[:, None, None]).astype(np.float32)


def reference_pil(img, geom, n, mean=MEAN, std=STD):
    """the same through Pillow itself: Image.crop(box).resize((ow, oh), BICUBIC), the window, transpose(FLIP_LEFT_RIGHT)"""
    from PIL import Image
    left, top, bw, bh, oh, ow, wtop, wleft, flip = geom
    im = Image.fromarray(img, "RGB").crop((left, top, left + bw, top + bh)).resize((ow, oh), Image.BICUBIC)
    im = im.crop((wleft, wtop, wleft + n, wtop + n))
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    x = np.asarray(im, dtype=np.float32) / np.float32(255.0)
    return ((x.transpose(2, 0, 1) - np.float32(mean)[:, None, None]) / np.float32(std)[:, None, None]).astype(np.float32)


def axis_range(in_size, out_size, first, n):
    """source coordinates [lo, lo + cnt) that the bicubic windows of outputs [first, first + n) touch and the window capacity
    (Pillow's precompute_coeffs: support = 2 * max(scale, 1), window = [int(c - s + 0.5), int(c + s + 0.5)) clamped); an axis
    that keeps its size is read directly: capacity 0"""
    if in_size == out_size:
        return first, n, 0
    scale = in_size / out_size
    support = 2.0 * max(scale, 1.0)
    lo = max(int((first + 0.5) * scale - support + 0.5), 0)
    hi = min(int((first + n - 1 + 0.5) * scale + support + 0.5), in_size)
    return lo, hi - lo, int(math.ceil(support)) * 2 + 1


def expected_plan(geoms, n):
    """independent restatement of uniir_image_batch_plan's layout: per image (kx, ky, y0, rows, x0, cols) and the offsets of
    its five workspace pieces, each rounded up to 256 bytes -> (list of dicts, workspace bytes, max rows)"""
    al = lambda x: (x + 255) & ~255
    ws, plans, max_rows = 0, [], 0
    for left, top, bw, bh, oh, ow, wtop, wleft, flip in geoms:
        x0, cols, kx = axis_range(bw, ow, wleft, n)
        y0, rows, ky = axis_range(bh, oh, wtop, n)
        p = dict(kx=kx, ky=ky, y0=y0, rows=rows, x0=x0, cols=cols)
        for name, size in (("bx_off", 8 * n), ("by_off", 8 * n), ("cx_off", 4 * n * kx), ("cy_off", 4 * n * ky),
                           ("tmp_off", 3 * rows * n)):
            p[name] = ws
            ws += al(size)
        plans.append(p)
        max_rows = max(max_rows, rows)
    return plans, ws, max_rows


def blip_train_draws(w, h, min_scale=0.5):
    """a copy of the draw sequence of blip_front.get_blip_transform's train_fn (torchvision RandomResizedCrop.get_params with
    scale (min_scale, 1), ratio (3/4, 4/3), then the flip coin) -> (left, top, box_w, box_h, flip)"""
    import random
    area = w * h
    box = None
    for _ in range(10):
        target = area * random.uniform(min_scale, 1.0)
        ratio = math.exp(random.uniform(math.log(3 / 4), math.log(4 / 3)))
        cw, ch = int(round(math.sqrt(target * ratio))), int(round(math.sqrt(target / ratio)))
        if 0 < cw <= w and 0 < ch <= h:
            top, left = random.randint(0, h - ch), random.randint(0, w - cw)
            box = (left, top, cw, ch)
            break
    fallback = box is None
    if fallback:
        r = w / h
        cw, ch = (w, int(round(w / (3 / 4)))) if r < 3 / 4 else ((int(round(h * (4 / 3))), h) if r > 4 / 3 else (w, h))
        box = ((w - cw) // 2, (h - ch) // 2, cw, ch)
    return box + (int(random.random() < 0.5),), fallback
