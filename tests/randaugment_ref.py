"""CPU restatement (numpy, no torch compute) of BLIP's training augmentation: the draw of the reference's
RandomAugment(2, 5, isPIL=True, augs=AUGS) (backbone/transform/randaugment.py, blip_transform.py:11-40) and its ten ops on an RGB
uint8 image [h][w][3].  It is the reference of uniir_image_augment_batch / uniir_image_preprocess_batch_aug and of the host path
in uniir_amd/randaugment.py; tests/test_randaugment_ref.py holds it to fixture G18 (the reference's own functions) for the draw
and the table ops, and to stated images and a derived bound for the warps, whose definition is the project's.

An op is (name, arg): arg is the enhance factor, the shear factor, the translate offset in pixels or the rotate angle in degrees.
`DEFECTS` is the set of planted faults that tests switch on to show that they bite; it is empty in every other use."""
import math

import numpy as np

AUGS = ["Identity", "AutoContrast", "Brightness", "Sharpness", "Equalize", "ShearX", "ShearY", "TranslateX", "TranslateY",
        "Rotate"]
# op codes of the aug table (include/uniir_hip.h [IMAGE]); AutoContrastPIL is never drawn unless asked for
CODES = {"Identity": 0, "AutoContrast": 1, "Equalize": 2, "Brightness": 3, "Sharpness": 4, "ShearX": 5, "ShearY": 6,
         "TranslateX": 7, "TranslateY": 8, "Rotate": 9, "AutoContrastPIL": 10}
FILL = 128
DEFECTS = set()     # of "centre", "forward", "floor", "neg_low", "last_bin"


class RandAugmentDraw:
    """draw() -> [(op, arg)] * N with exactly the reference's np.random calls: choice(augs, N), then per op one random() for the
    skip (> 0.5 skips: the op comes out as Identity) and, for shear / translate / rotate, one more for the sign"""

    def __init__(self, N=2, M=5, augs=None, pil_autocontrast=False):
        self.N, self.M, self.augs, self.pil_autocontrast = N, M, list(AUGS if augs is None else augs), pil_autocontrast

    def draw(self):
        out = []
        for name in np.random.choice(self.augs, self.N):
            name = str(name)
            if np.random.random() > 0.5:
                out.append(("Identity", 0.0))
                continue
            level = self.M / 10
            if name in ("ShearX", "ShearY"):
                arg = level * 0.3
                if np.random.random() > 0.5:
                    arg = -arg
            elif name in ("TranslateX", "TranslateY"):
                arg = level * float(10)
                if np.random.random() > 0.5:
                    arg = -arg
            elif name == "Rotate":
                arg = level * 30
                if np.random.random() < 0.5:
                    arg = -arg
            elif name in ("Brightness", "Sharpness"):
                arg = level * 1.8 + 0.1
            else:
                arg = 0.0
            if name == "AutoContrast" and self.pil_autocontrast:
                name = "AutoContrastPIL"
            out.append((name, float(arg)))
        return out


# ---------------------------------------------------------------------------------------------------------------------------
# table ops: a 256-entry table per channel, or None for a channel that stays as it is
# ---------------------------------------------------------------------------------------------------------------------------
def autocontrast_table(ch, pil=False):
    lo, hi = int(ch.min()), int(ch.max())
    if hi <= lo:
        return None
    scale = 255.0 / (hi - lo)                                    # fp64 throughout; the products are rounded before the sum
    off = -lo * scale if (pil or "neg_low" in DEFECTS) else ((256 - lo) % 256) * scale    # the reference negates a uint8
    t = np.arange(256, dtype=np.float64) * scale + off
    return np.clip(t, 0.0, 255.0).astype(np.int64).astype(np.uint8)


def equalize_table(ch):
    hist = np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)
    last = 255 if "last_bin" in DEFECTS else int(np.nonzero(hist)[0][-1])
    step = int(hist.sum() - hist[last]) // 255
    if step == 0:
        return None
    n = np.empty(256, dtype=np.int64)
    n[0] = step // 2
    n[1:] = hist[:-1]
    return np.minimum(np.cumsum(n) // step, 255).astype(np.uint8)


def brightness_table(factor):
    t = np.arange(256, dtype=np.float32) * np.float32(factor)
    return np.trunc(np.clip(t, np.float32(0), np.float32(255))).astype(np.uint8)


def _per_channel(img, table_of):
    out = img.copy()
    for c in range(img.shape[2]):
        t = table_of(img[:, :, c])
        if t is not None:
            out[:, :, c] = t[img[:, :, c]]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# warps: forward matrix -> fp64 inverse on the host -> 1/1024 fixed-point coordinates on a 1/32 grid, 15-bit bilinear weights
# ---------------------------------------------------------------------------------------------------------------------------
def forward_matrix(name, arg, h, w):
    if name == "ShearX":
        return [[1.0, float(np.float32(arg)), 0.0], [0.0, 1.0, 0.0]]
    if name == "ShearY":
        return [[1.0, 0.0, 0.0], [float(np.float32(arg)), 1.0, 0.0]]
    if name == "TranslateX":
        return [[1.0, 0.0, float(np.float32(-arg))], [0.0, 1.0, 0.0]]
    if name == "TranslateY":
        return [[1.0, 0.0, 0.0], [0.0, 1.0, float(np.float32(-arg))]]
    assert name == "Rotate", name
    cx, cy = ((w - 1) / 2, (h - 1) / 2) if "centre" in DEFECTS else (w / 2, h / 2)
    rad = arg * (math.pi / 180.0)
    a, b = math.cos(rad), math.sin(rad)
    return [[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]]


def invert(m):
    """2x3 affine inverse in fp64, every product rounded before it is summed"""
    (a00, a01, a02), (a10, a11, a12) = m
    d = a00 * a11 - a01 * a10
    d = 1.0 / d if d != 0 else 0.0
    i00, i11 = a11 * d, a00 * d
    i01, i10 = a01 * -d, a10 * -d
    return [[i00, i01, -i00 * a02 - i01 * a12], [i10, i11, -i10 * a02 - i11 * a12]]


def inverse_matrix(name, arg, h, w):
    m = forward_matrix(name, arg, h, w)
    return m if "forward" in DEFECTS else invert(m)


def _fix(v):
    r = np.floor(v) if "floor" in DEFECTS else np.rint(v)            # rint: half to even
    return np.clip(r, -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)


def bilinear_weights():
    """[32][32][4] int weights of the fractions (fy, fx) for the cells (0,0) (0,1) (1,0) (1,1): rint(wy * wx * 32768) in
    float32, then made to sum to 32768: a shortfall goes to the largest, an excess comes off the smallest"""
    tab = np.zeros((32, 32, 4), dtype=np.int64)
    for fy in range(32):
        wy = (np.float32(1) - np.float32(fy) / np.float32(32), np.float32(fy) / np.float32(32))
        for fx in range(32):
            wx = (np.float32(1) - np.float32(fx) / np.float32(32), np.float32(fx) / np.float32(32))
            w = [int(np.rint(np.float32(wy[i] * wx[j]) * np.float32(32768))) for i in (0, 1) for j in (0, 1)]
            diff = 32768 - sum(w)
            if diff > 0:
                w[w.index(max(w))] += diff
            elif diff < 0:
                w[w.index(min(w))] += diff
            tab[fy, fx] = w
    return tab


_WEIGHTS = bilinear_weights()


def warp_coords(inv, h, w):
    """-> (X, Y) int64 [h][w]: source coordinates of every destination pixel in 1/32 pixel"""
    (m00, m01, m02), (m10, m11, m12) = inv
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    X = (_fix((m01 * y + m02) * 1024.0) + 16 + _fix(m00 * x * 1024.0)) >> 5
    Y = (_fix((m11 * y + m12) * 1024.0) + 16 + _fix(m10 * x * 1024.0)) >> 5
    return X, Y


def warp(img, inv):
    h, w = img.shape[:2]
    X, Y = warp_coords(inv, h, w)
    sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
    wts = _WEIGHTS[fy, fx]                                           # [h][w][4]
    acc = np.zeros(img.shape, dtype=np.int64)
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        yy, xx = sy + dy, sx + dx
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        p = np.where(inside[:, :, None], img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), FILL)
        acc += p * wts[:, :, k, None]
    return ((acc + 16384) >> 15).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------------------
# sharpness
# ---------------------------------------------------------------------------------------------------------------------------
def smooth(img):
    """the 3x3 filter (1 ... 5 ... 1) / 13 in float32, taps added in row-major order, reflect-101 border, half-even, saturated"""
    k, kc = np.float32(1) / np.float32(13), np.float32(5) / np.float32(13)
    h, w = img.shape[:2]
    iy = np.array([1 if h > 1 else 0] + list(range(h)) + [h - 2 if h > 1 else 0])
    ix = np.array([1 if w > 1 else 0] + list(range(w)) + [w - 2 if w > 1 else 0])
    p = img[iy][:, ix].astype(np.float32)
    acc = np.zeros(img.shape, dtype=np.float32)
    for dy in range(3):
        for dx in range(3):
            acc = acc + p[dy:dy + h, dx:dx + w] * (kc if dy == 1 and dx == 1 else k)
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def sharpness(img, factor):
    if factor == 1.0:
        return img.copy()
    deg = smooth(img)
    if factor == 0.0:
        return deg
    out = img.copy()
    d, x = deg[1:-1, 1:-1].astype(np.float32), img[1:-1, 1:-1].astype(np.float32)
    v = d + np.float32(factor) * (x - d)
    v = np.clip(np.trunc(v), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)      # astype(uint8): to int32, the low 8 bits kept
    out[1:-1, 1:-1] = (v & 255).astype(np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def apply_op(img, name, arg=0.0):
    if name == "Identity":
        return img.copy()
    if name in ("AutoContrast", "AutoContrastPIL"):
        return _per_channel(img, lambda ch: autocontrast_table(ch, pil=name == "AutoContrastPIL"))
    if name == "Equalize":
        return _per_channel(img, equalize_table)
    if name == "Brightness":
        return brightness_table(arg)[img]
    if name == "Sharpness":
        return sharpness(img, arg)
    return warp(img, inverse_matrix(name, arg, img.shape[0], img.shape[1]))


def apply_ops(img, ops):
    for name, arg in ops:
        img = apply_op(img, name, arg)
    return img


# ---------------------------------------------------------------------------------------------------------------------------
# test images shared by the CPU and the GPU tests
# ---------------------------------------------------------------------------------------------------------------------------
def lut_cases():
    """name -> RGB uint8 image, 16 x 16 and 19 x 19: the channel shapes the table ops branch on.  Fixture G18 stores the
    reference's outputs on exactly these (tests/golden/make_golden_randaugment.py imports this function)."""
    out = {}
    for n in (16, 19):
        rng = np.random.default_rng(1800 + n)
        full = rng.integers(0, 256, (n, n, 3), dtype=np.uint8)
        full[0, 0], full[0, 1] = 0, 255                              # every channel: min 0, max 255
        out[f"full{n}"] = full
        a = rng.integers(13, 201, (n, n, 3), dtype=np.uint8)         # min > 0 (the wrapped offset), max < 255
        a[0, 0], a[0, 1] = 13, 200
        out[f"minpos{n}"] = a
        b = rng.integers(0, 180, (n, n, 3), dtype=np.uint8)          # min 0, max < 255: the stretch as intended
        b[0, 0], b[0, 1] = 0, 179
        out[f"lowmax{n}"] = b
        flat = np.empty((n, n, 3), dtype=np.uint8)                   # flat channels (0, 77, 255): hi <= lo, step 0
        flat[:] = (0, 77, 255)
        out[f"flat{n}"] = flat
        two = np.where(rng.random((n, n, 3)) < 0.3, 40, 190).astype(np.uint8)     # two values per channel
        two[0, 0], two[0, 1] = 40, 190
        two[:, :, 2] = np.where(two[:, :, 2] == 40, 0, 255)
        out[f"two{n}"] = two
        z = np.full((n, n, 3), 90, dtype=np.uint8)                   # nearly flat: fewer than 255 pixels outside the last
        z.reshape(-1, 3)[:200, 0] = 10                               # nonzero bin -> equalize's step is 0 (channel 0 at n = 16:
        z.reshape(-1, 3)[:254, 1] = rng.integers(0, 90, 254)         # 200 // 255; channel 1: 254 // 255); channel 2 has 255
        z.reshape(-1, 3)[:255, 2] = rng.integers(0, 90, 255)         # of them: step 1, the smallest that equalizes
        out[f"step0_{n}"] = z
    return out


def smooth_image(n, amp=(100.0, -80.0, 60.0)):
    """a smooth image that runs into the fill value at its edges, so that the image continued by the fill has a small
    difference between any two neighbouring pixels (max_step measures it)"""
    y, x = np.mgrid[0:n, 0:n].astype(np.float64)
    u, v = np.pi * (x + 1) / (n + 1), np.pi * (y + 1) / (n + 1)
    chans = [FILL + a * np.sin(u) * np.sin(v) + 0.25 * a * np.sin(2 * u) * np.sin((c + 1) * v) for c, a in enumerate(amp)]
    return np.clip(np.rint(np.stack(chans, axis=2)), 0, 255).astype(np.uint8)


def max_step(img):
    """largest difference between horizontal or vertical neighbours of the image continued by the fill value"""
    p = np.pad(img.astype(np.int64), ((1, 1), (1, 1), (0, 0)), constant_values=FILL)
    return int(max(np.abs(np.diff(p, axis=0)).max(), np.abs(np.diff(p, axis=1)).max()))


def bilinear_fp64(img, inv):
    """fp64 bilinear interpolation of the same transform, the fill outside: the smooth-image bound's reference"""
    h, w = img.shape[:2]
    (m00, m01, m02), (m10, m11, m12) = inv
    x = np.arange(w, dtype=np.float64)[None, :]
    y = np.arange(h, dtype=np.float64)[:, None]
    sx, sy = m00 * x + m01 * y + m02, m10 * x + m11 * y + m12
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0)[:, :, None], (sy - y0)[:, :, None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def px(yy, xx):
        inside = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        return np.where(inside[:, :, None], img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.float64), float(FILL))

    return ((1 - fy) * ((1 - fx) * px(y0, x0) + fx * px(y0, x0 + 1)) + fy * ((1 - fx) * px(y0 + 1, x0) + fx * px(y0 + 1, x0 + 1)))
