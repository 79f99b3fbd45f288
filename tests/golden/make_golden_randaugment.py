"""G18: what the reference's RandomAugment draws and what its table ops compute, captured by IMPORTING THE REFERENCE module
(/root/reference/src/models/uniir_blip/backbone/transform/randaugment.py, read-only) in the build container.  The module imports
OpenCV, which is not installed; it runs here under a stand-in of exactly three functions -- split (channel list), merge (stack) and
calcHist (np.bincount(..., minlength=256) as float32 [256][1]) -- which is all that autocontrast_func, equalize_func and
brightness_func use.  rotate_func, the shears, the translates and sharpness_func call warpAffine / getRotationMatrix2D / filter2D:
they cannot run and are NOT in the fixture (parity of those ops with OpenCV itself is unpinned).

 (a) draws: for 8 seeds x 16 consecutive images and M in (5, 8), the (name, argument) sequence that
     RandomAugment(2, M, isPIL=True, augs=<BLIP's ten>) hands to its op functions (func_dict entries replaced by recorders; an op
     that the policy skips calls nothing and is absent), and a hash of the np.random state after every image;
 (b) pixels: autocontrast_func and equalize_func on the images of tests/randaugment_ref.lut_cases(), brightness_func for the
     factors 0.1, 0.64, 1.0, 1.9 on two of them.
    python tests/golden/make_golden_randaugment.py"""
import hashlib
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from randaugment_ref import AUGS, lut_cases  # noqa: E402  (the input images only)

REF = "/root/reference/src/models/uniir_blip/backbone/transform/randaugment.py"
SEEDS, IMAGES, LEVELS = list(range(8)), 16, (5, 8)
FACTORS = (0.1, 0.64, 1.0, 1.9)

cv2 = types.ModuleType("cv2")
cv2.split = lambda img: [img[:, :, c] for c in range(img.shape[2])]
cv2.merge = lambda chans: np.stack(chans, axis=2)
cv2.calcHist = lambda imgs, ch, mask, size, rng: np.bincount(imgs[0].reshape(-1), minlength=256).astype(np.float32).reshape(256, 1)
sys.modules["cv2"] = cv2
spec = importlib.util.spec_from_file_location("reference_randaugment", REF)
ra = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ra)


def state_hash():
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return hashlib.sha256(keys.tobytes() + str((kind, int(pos), int(has_gauss), float(cached))).encode()).hexdigest()


out = {"numpy_version": np.array(np.__version__)}
# (b) first: the real functions, before the recorders replace them
cases = lut_cases()
out["case_names"] = np.array(sorted(cases))
for name, img in cases.items():
    out[f"{name}_img"] = img
    out[f"{name}_autocontrast"] = ra.autocontrast_func(img)
    out[f"{name}_equalize"] = ra.equalize_func(img)
out["brightness_cases"] = np.array(["full16", "full19"])
out["brightness_factors"] = np.array(FACTORS)
for name in ("full16", "full19"):
    for f in FACTORS:
        out[f"{name}_brightness_{f}"] = ra.brightness_func(cases[name], f)

# (a) recorders in place of every op function
calls = []


def recorder(name):
    def fn(img, *args):
        calls.append([name, float(args[0]) if args and not isinstance(args[0], tuple) else 0.0])
        return img
    return fn


for name in list(ra.func_dict):
    ra.func_dict[name] = recorder(name)
draws = {}
img = np.zeros((8, 8, 3), dtype=np.uint8)
for M in LEVELS:
    policy = ra.RandomAugment(2, M, isPIL=True, augs=list(AUGS))
    for seed in SEEDS:
        np.random.seed(seed)
        rows = []
        for _ in range(IMAGES):
            del calls[:]
            policy(img)
            rows.append({"ops": [list(c) for c in calls], "state": state_hash()})
        draws[f"M{M}_seed{seed}"] = rows
out["draws_json"] = np.array(json.dumps(draws))
out["augs"] = np.array(AUGS)
path = os.path.join(HERE, "g18_randaugment.npz")
np.savez_compressed(path, **out)
print("wrote", path, os.path.getsize(path), "bytes;", "seed 3, M 5:", [r["ops"] for r in draws["M5_seed3"][:3]])
