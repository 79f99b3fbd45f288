"""BLIP's training augmentation (upstream backbone/transform/randaugment.py as blip_transform.py:11-40 configures it:
RandomAugment(2, 5, isPIL=True, augs=AUGS)): the draw, and the ten ops on the host in numpy.

The draw always runs on the host (loader workers) and makes exactly the reference's np.random calls.  The ops run either here
(blip_front.get_blip_transform(..., randaugment=(N, M))) or on the device from the drawn list (blip_front.RawBlipTransform ->
clip_front.RawImageBatch -> uniir_image_preprocess_batch_aug); both give the same bytes (tests/test_randaugment_gpu.py).  The
table ops compute what the reference computes (fixture G18), the reference's uint8 wrap in AutoContrast included; the warps and
the 3x3 filter follow the project's own definition (written after OpenCV's published fixed-point scheme --
OpenCV is not installed, parity with it is unpinned).

An op is (name, arg): arg = the enhance factor, the shear factor, the translate offset in pixels or the angle in degrees."""
import math

import numpy as np

AUGS = ("Identity", "AutoContrast", "Brightness", "Sharpness", "Equalize", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
# op codes of include/uniir_hip.h [IMAGE]
OP_CODES = {"Identity": 0, "AutoContrast": 1, "Equalize": 2, "Brightness": 3, "Sharpness": 4, "ShearX": 5, "ShearY": 6,
            "TranslateX": 7, "TranslateY": 8, "Rotate": 9, "AutoContrastPIL": 10}
MAX_SLOTS = 4
_FILL = 128


class RandAugmentDraw:
    """draw() -> N (op, arg) pairs.  np.random calls, in the reference's order and number: choice(augs, N); per op random() > 0.5
    skips it (it comes out as Identity); shear and translate take one more random() (> 0.5: negative), rotate too (< 0.5:
    negative).  pil_autocontrast=True maps AutoContrast to Pillow's formula instead of the reference's."""

    def __init__(self, N=2, M=5, augs=AUGS, pil_autocontrast=False):
        if not 0 < N <= MAX_SLOTS:
            raise ValueError(f"N must be in 1 .. {MAX_SLOTS}")
        unknown = [a for a in augs if a not in OP_CODES]
        if unknown:
            raise ValueError(f"ops not carried: {unknown}")
        self.N, self.M, self.augs, self.pil_autocontrast = N, M, list(augs), pil_autocontrast

    def draw(self):
        ops, level = [], self.M / 10
        for name in np.random.choice(self.augs, self.N):
            name = str(name)
            if np.random.random() > 0.5:
                ops.append(("Identity", 0.0))
                continue
            arg = 0.0
            if name in ("Brightness", "Sharpness"):
                arg = level * 1.8 + 0.1
            elif name in ("ShearX", "ShearY"):
                arg = level * 0.3
                arg = -arg if np.random.random() > 0.5 else arg
            elif name in ("TranslateX", "TranslateY"):
                arg = level * 10.0
                arg = -arg if np.random.random() > 0.5 else arg
            elif name == "Rotate":
                arg = level * 30
                arg = -arg if np.random.random() < 0.5 else arg
            elif name == "AutoContrast" and self.pil_autocontrast:
                name = "AutoContrastPIL"
            ops.append((name, float(arg)))
        return ops


def _channel_table(ch, name):
    """the 256-entry table of a histogram op for one channel, None when the channel stays as it is"""
    hist = np.bincount(ch.ravel(), minlength=256)
    present = np.flatnonzero(hist)
    lo, hi = int(present[0]), int(present[-1])
    if name == "Equalize":
        step = int(ch.size - hist[hi]) // 255
        if step == 0:
            return None
        below = np.concatenate(([0], np.cumsum(hist[:-1])))
        return np.minimum((step // 2 + below) // step, 255).astype(np.uint8)
    if hi <= lo:
        return None
    scale = 255.0 / (hi - lo)
    off = -lo * scale if name == "AutoContrastPIL" else ((256 - lo) % 256) * scale     # the reference negates a uint8
    return np.clip(np.arange(256.0) * scale + off, 0.0, 255.0).astype(np.int64).astype(np.uint8)


def inverse_matrix(name, arg, h, w):
    """forward matrix of a warp op (shear / translate entries rounded to float32, rotation about (w / 2, h / 2)) -> fp64 inverse"""
    a00, a01, a02, a10, a11, a12 = 1.0, 0.0, 0.0, 0.0, 1.0, 0.0
    if name == "ShearX":
        a01 = float(np.float32(arg))
    elif name == "ShearY":
        a10 = float(np.float32(arg))
    elif name == "TranslateX":
        a02 = float(np.float32(-arg))
    elif name == "TranslateY":
        a12 = float(np.float32(-arg))
    else:
        cx, cy, rad = w / 2, h / 2, arg * (math.pi / 180.0)
        a, b = math.cos(rad), math.sin(rad)
        a00, a01, a02, a10, a11, a12 = a, b, (1 - a) * cx - b * cy, -b, a, b * cx + (1 - a) * cy
    d = a00 * a11 - a01 * a10
    d = 1.0 / d if d != 0 else 0.0
    i00, i11, i01, i10 = a11 * d, a00 * d, a01 * -d, a10 * -d
    return (i00, i01, -i00 * a02 - i01 * a12, i10, i11, -i10 * a02 - i11 * a12)


def _fix(v):
    return np.clip(np.rint(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def _warp(img, m):
    h, w = img.shape[:2]
    x, y = np.arange(w, dtype=np.float64)[None, :], np.arange(h, dtype=np.float64)[:, None]
    X = (_fix((m[1] * y + m[2]) * 1024.0) + 16 + _fix(m[0] * x * 1024.0)) >> 5
    Y = (_fix((m[4] * y + m[5]) * 1024.0) + 16 + _fix(m[3] * x * 1024.0)) >> 5
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    acc = np.zeros(img.shape, dtype=np.int64)
    # rint(wy * wx * 32768) of 1/32 fractions are exact integers of sum 32768: the sum correction of the definition never applies
    for dy, dx, wt in ((0, 0, (32 - fy) * (32 - fx)), (0, 1, (32 - fy) * fx), (1, 0, fy * (32 - fx)), (1, 1, fy * fx)):
        yy, xx = sy + dy, sx + dx
        inside = ((yy >= 0) & (yy < h) & (xx >= 0) & (xx < w))[:, :, None]
        acc += np.where(inside, img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)], _FILL) * (wt * 32)[:, :, None]
    return ((acc + 16384) >> 15).astype(np.uint8)


def _sharpness(img, factor):
    if factor == 1.0:
        return img
    k, kc = np.float32(1) / np.float32(13), np.float32(5) / np.float32(13)
    h, w = img.shape[:2]
    p = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="reflect").astype(np.float32) if min(h, w) > 1 else \
        np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="edge").astype(np.float32)
    acc = np.zeros(img.shape, dtype=np.float32)
    for dy in range(3):
        for dx in range(3):
            acc = acc + p[dy:dy + h, dx:dx + w] * (kc if dy == dx == 1 else k)
    deg = np.clip(np.rint(acc), 0, 255).astype(np.uint8)
    if factor == 0.0:
        return deg
    out = img.copy()
    d, x = deg[1:-1, 1:-1].astype(np.float32), img[1:-1, 1:-1].astype(np.float32)
    v = np.clip(np.trunc(d + np.float32(factor) * (x - d)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
    out[1:-1, 1:-1] = (v & 255).astype(np.uint8)
    return out


def apply_ops(img, ops):
    """RGB uint8 [h][w][3] -> the same after every (name, arg) of `ops` in order"""
    for name, arg in ops:
        if name == "Identity":
            continue
        if name in ("AutoContrast", "AutoContrastPIL", "Equalize"):
            out = img.copy()
            for c in range(img.shape[2]):
                t = _channel_table(img[:, :, c], name)
                if t is not None:
                    out[:, :, c] = t[img[:, :, c]]
            img = out
        elif name == "Brightness":
            t = np.arange(256, dtype=np.float32) * np.float32(arg)
            img = np.trunc(np.clip(t, np.float32(0), np.float32(255))).astype(np.uint8)[img]
        elif name == "Sharpness":
            img = _sharpness(img, arg)
        elif name in OP_CODES:
            img = _warp(img, inverse_matrix(name, arg, img.shape[0], img.shape[1]))
        else:
            raise ValueError(f"op not carried: {name}")
    return img


def op_arrays(ops_per_image):
    """[(name | code, arg)] per image (None = none) -> (int32 [count][slots], float64 [count][slots], slots) for
    uniir_image_aug_plan; shorter lists are padded with Identity"""
    lists = [list(o) if o else [] for o in ops_per_image]
    slots = max([len(o) for o in lists] + [0])
    if slots > MAX_SLOTS:
        raise ValueError(f"at most {MAX_SLOTS} ops per image")
    codes, args = np.zeros((len(lists), max(slots, 1)), dtype=np.int32), np.zeros((len(lists), max(slots, 1)), dtype=np.float64)
    for i, o in enumerate(lists):
        for k, (name, arg) in enumerate(o):
            codes[i, k] = OP_CODES[name] if isinstance(name, str) else int(name)
            args[i, k] = float(arg)
    return codes[:, :slots].copy(), args[:, :slots].copy(), slots
