"""The numpy restatement of BLIP's RandomAugment (tests/randaugment_ref.py) against what can be pinned on a CPU:
  * fixture G18 (the reference's own module under a three-function stand-in for OpenCV): every recorded draw with the np.random
    state after it, and the bytes of autocontrast_func / equalize_func / brightness_func on every table edge case;
  * Pillow for the AutoContrastPIL op code;
  * for the warps, whose definition is the project's own: images stated pixel by pixel, and on smooth
    images a bound from the fp64 bilinear interpolation of the same transform, derived below and held on every pixel;
  * five planted defects, each of which must fail at least one of the checks above."""
import hashlib
import json
import os

import numpy as np
import pytest

import randaugment_ref as R

G18 = np.load(os.path.join(os.path.dirname(__file__), "golden", "g18_randaugment.npz"))
DRAWS = json.loads(str(G18["draws_json"]))
CASES = R.lut_cases()


def _state_hash():
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return hashlib.sha256(keys.tobytes() + str((kind, int(pos), int(has_gauss), float(cached))).encode()).hexdigest()


# ---- the checks, as functions, so that the planted-defect test can run them again -------------------------------------------
def check_lut_cases():
    assert sorted(CASES) == [str(s) for s in G18["case_names"]] and len(CASES) == 12
    for name, img in CASES.items():
        assert np.array_equal(img, G18[f"{name}_img"]), name
        assert np.array_equal(R.apply_op(img, "AutoContrast"), G18[f"{name}_autocontrast"]), name
        assert np.array_equal(R.apply_op(img, "Equalize"), G18[f"{name}_equalize"]), name
    for name in G18["brightness_cases"]:
        for f in G18["brightness_factors"]:
            assert np.array_equal(R.apply_op(CASES[str(name)], "Brightness", float(f)), G18[f"{name}_brightness_{f}"]), (name, f)


def _shifted(img, dx, dy):
    """out[y][x] = img[y - dy][x - dx], the fill where that is outside"""
    n = img.shape[0]
    out = np.full_like(img, R.FILL)
    ys, xs = np.arange(n) - dy, np.arange(n) - dx
    oky, okx = (ys >= 0) & (ys < n), (xs >= 0) & (xs < n)
    out[np.ix_(oky, okx)] = img[np.ix_(ys[oky], xs[okx])]
    return out


def check_exact_warps():
    rng = np.random.default_rng(5)
    for n in (16, 19):
        img = rng.integers(0, 256, (n, n, 3), dtype=np.uint8)
        # the reference's translate_x_func(img, o) builds [[1, 0, -o]]: the content moves by o pixels to the LEFT
        for o in (5.0, -5.0):
            assert np.array_equal(R.apply_op(img, "TranslateX", o), _shifted(img, -int(o), 0)), (n, o)
            assert np.array_equal(R.apply_op(img, "TranslateY", o), _shifted(img, 0, -int(o))), (n, o)
        for name in ("ShearX", "ShearY", "Rotate"):
            assert np.array_equal(R.apply_op(img, name, 0.0), img), (n, name)
    for n in (16, 24):          # even n: rotation by 180 degrees about (n / 2, n / 2) maps (x, y) to (n - x, n - y)
        img = rng.integers(0, 256, (n, n, 3), dtype=np.uint8)
        ext = np.full((n + 1, n + 1, 3), R.FILL, dtype=np.uint8)        # row and column n count as the fill
        ext[:n, :n] = img
        idx = n - np.arange(n)
        assert np.array_equal(R.apply_op(img, "Rotate", 180.0), ext[np.ix_(idx, idx)]), n
    # rint, not floor, of the matrix terms: an offset of 15.75 / 1024 pixel rounds to 16 / 1024, which with the rounding
    # constant 16 reaches the first 1/32 step -> a 31 : 1 blend with the right neighbour (floor stays on the pixel)
    n = 16
    img = np.zeros((n, n, 3), dtype=np.uint8)
    img[:, :8] = (32 * np.arange(8, dtype=np.uint8))[None, :, None]
    want = img.copy()
    want[:, :7] += 1                            # (32 x * 31 + 32 (x + 1)) * 1024 + 16384 >> 15 = 32 x + 1
    want[:, 7] = (224 * 31 * 1024 + 0 + 16384) >> 15
    want[:, 15] = (0 * 31 + 128) * 1024 + 16384 >> 15                   # the right neighbour of the last column is the fill
    assert np.array_equal(R.apply_op(img, "TranslateX", 15.75 / 1024), want)


def warp_bound(step):
    """|fixed-point warp - fp64 bilinear| on an image whose neighbours (the fill outside included) differ by at most `step`.
    Each source coordinate is off by at most 1/1024 (two matrix terms rounded to 1/1024, 1/2048 each) + 1/64 (the sum rounded
    to the 1/32 grid); the bilinear surface changes by at most `step` per unit along either axis, so the value moves by at most
    2 * step * (1/64 + 1/1024).  The 15-bit weights of 1/32 fractions are exact; the last shift rounds: + 1/2."""
    return 2.0 * step * (1.0 / 64 + 1.0 / 1024) + 0.5 + 1e-9


def check_smooth_bound():
    for n in (24, 32):
        img = R.smooth_image(n)
        step = R.max_step(img)
        assert 0 < step <= 24, step          # amplitude 100 over n + 1 = 25 pixels: pi * 100 / 25 * 1.5
        for name, arg in (("Rotate", 15.0), ("Rotate", -15.0), ("Rotate", 77.0), ("ShearX", 0.15), ("ShearX", -0.15), ("ShearY", 0.15),
                          ("ShearY", -0.24), ("TranslateX", 3.3), ("TranslateY", -2.7)):
            got = R.apply_op(img, name, arg).astype(np.float64)
            want = R.bilinear_fp64(img, R.invert(R.forward_matrix(name, arg, n, n)))
            err = np.abs(got - want).max()          # every pixel, the ones next to the fill included
            assert err <= warp_bound(step), (n, name, arg, err, warp_bound(step))


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_table_ops_equal_the_reference_byte_for_byte():
    check_lut_cases()


def test_the_reference_autocontrast_wraps_and_the_fixture_shows_it():
    """min 13 > 0: the reference's uint8 negation turns the offset positive and everything saturates -- not Pillow's result"""
    want = G18["minpos16_autocontrast"]
    assert (want == 255).all()
    assert np.array_equal(G18["flat19_autocontrast"], CASES["flat19"]) and np.array_equal(G18["flat16_equalize"], CASES["flat16"])
    assert np.array_equal(G18["step0_16_equalize"][:, :, :2], CASES["step0_16"][:, :, :2])          # step 0: unchanged
    assert not np.array_equal(G18["step0_16_equalize"][:, :, 2], CASES["step0_16"][:, :, 2])        # step 1: equalized


@pytest.mark.parametrize("M", [5, 8])
def test_draw_reproduces_every_recorded_sequence_and_state(M):
    draw = R.RandAugmentDraw(2, M)
    assert [str(a) for a in G18["augs"]] == R.AUGS
    seen = set()
    for seed in range(8):
        rows = DRAWS[f"M{M}_seed{seed}"]
        assert len(rows) == 16
        np.random.seed(seed)
        for i, row in enumerate(rows):
            ops = draw.draw()
            assert len(ops) == 2
            # a skipped op calls nothing in the reference and is Identity here; a drawn Identity is Identity in both
            got = [[n, a] for n, a in ops if n != "Identity"]
            want = [[n, a] for n, a in row["ops"] if n != "Identity"]
            assert got == want, (seed, i, ops, row["ops"])
            assert _state_hash() == row["state"], (seed, i)
            seen.update(n for n, _ in want)
    assert seen == set(R.AUGS) - {"Identity"}
    if M == 5:
        first = [[n for n, a in r["ops"]] for r in DRAWS["M5_seed3"][:3]]
        assert first == [["Rotate"], ["Sharpness", "Rotate"], ["Equalize", "TranslateX"]]
        assert R.RandAugmentDraw(2, 5).M / 10 * 1.8 + 0.1 == 1.0           # Brightness and Sharpness are the identity at level 5


def test_autocontrast_pil_equals_pillow():
    from PIL import Image, ImageOps
    rng = np.random.default_rng(9)
    imgs = list(CASES.values()) + [rng.integers(lo, hi + 1, (21, 17, 3), dtype=np.uint8) for lo, hi in ((3, 250), (100, 101), (0, 7),
                                                                                                        (254, 255), (77, 203))]
    for img in imgs:
        want = np.asarray(ImageOps.autocontrast(Image.fromarray(img, "RGB")))
        assert np.array_equal(R.apply_op(img, "AutoContrastPIL"), want)
    draw = R.RandAugmentDraw(2, 5, augs=["AutoContrast"], pil_autocontrast=True)
    np.random.seed(0)
    assert {n for _ in range(8) for n, _ in draw.draw()} == {"Identity", "AutoContrastPIL"}


def test_bilinear_weights_are_exact_and_sum_to_one():
    """the fractions are multiples of 1/32, so rint(wy * wx * 32768) = (32 - fy)(32 - fx) * 32 ... exactly and the sum correction
    of the definition never moves a weight: the kernel computes the closed form"""
    tab = R.bilinear_weights()
    fy, fx = np.mgrid[0:32, 0:32]
    closed = np.stack([(32 - fy) * (32 - fx), (32 - fy) * fx, fy * (32 - fx), fy * fx], axis=2) * 32
    assert np.array_equal(tab, closed) and (tab.sum(axis=2) == 32768).all()


def test_warps_give_the_stated_images():
    check_exact_warps()


def test_warps_stay_within_the_derived_bound_of_fp64_bilinear():
    check_smooth_bound()


def test_sharpness_definition():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (19, 19, 3), dtype=np.uint8)
    assert np.array_equal(R.sharpness(img, 1.0), img)
    flat = np.full((16, 16, 3), 91, dtype=np.uint8)
    for f in (0.0, 0.37, 1.9):                      # 9 taps of 91 in fp32 round back to 91
        assert np.array_equal(R.sharpness(flat, f), flat), f
    deg = R.sharpness(img, 0.0)
    # independent fp64 filter with the reflect-101 border: the fp32 sum may differ from it only at rounding ties
    pad = np.pad(img.astype(np.float64), ((1, 1), (1, 1), (0, 0)), mode="reflect")
    ref = sum(pad[dy:dy + 19, dx:dx + 19] * (5.0 if dy == dx == 1 else 1.0) for dy in range(3) for dx in range(3)) / 13.0
    assert np.abs(deg.astype(np.float64) - ref).max() <= 0.5 + 1e-4
    out = R.sharpness(img, 1.9)
    assert np.array_equal(out[0], img[0]) and np.array_equal(out[:, -1], img[:, -1])          # the border keeps the input
    d, x = deg[1:-1, 1:-1].astype(np.float32), img[1:-1, 1:-1].astype(np.float32)
    v = np.trunc(d + np.float32(1.9) * (x - d)).astype(np.int64)
    assert (v < 0).any() and (v > 255).any()                    # both wrap directions occur: 300.7 -> 44, -3.2 -> 253
    assert np.array_equal(out[1:-1, 1:-1], (v % 256).astype(np.uint8))
    assert np.array_equal(np.array([300.7, -3.2], dtype=np.float32).astype(np.int32) & 255, [44, 253])


DEFECT_CHECKS = {"centre": check_exact_warps, "forward": check_exact_warps, "floor": check_exact_warps, "neg_low": check_lut_cases,
                 "last_bin": check_lut_cases}


@pytest.mark.parametrize("defect", sorted(DEFECT_CHECKS))
def test_planted_defects_fail(defect):
    """centre (W - 1) / 2; the forward matrix used as the inverse; floor for rint; the sign of -low 'fixed'; the last bin instead of
    the last nonzero bin dropped in Equalize -- each must be caught by the check named for it, which passes without it"""
    assert not R.DEFECTS
    DEFECT_CHECKS[defect]()
    R.DEFECTS.add(defect)
    try:
        with pytest.raises(AssertionError):
            DEFECT_CHECKS[defect]()
    finally:
        R.DEFECTS.clear()
