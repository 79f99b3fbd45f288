"""uniir_gemm_wgrad_side_plan (include/uniir_hip.h, csrc/gemm.hip) on the CPU: the chunk arithmetic of the weight-gradient launch with
LayerNorm side rows is host arithmetic.  Over the row counts and tile counts that tests/test_abi.py sweeps for the split rule, and
every count of side compute units, a returned plan satisfies the conditions of the launch -- chunks divide over the product's
workgroups, every K range keeps >= 16 steps of 64 rows and none is empty -- and is the smallest such split count; 0 is returned only
where no count up to 64 satisfies them.  The slab-room condition needs a descriptor and is exercised on the GPU."""
import ctypes as C

ROWS = (1, 63, 1023, 1024, 1025, 4096, 33280, 35000, 263168, 590848)
NCU = 256


def _ok(rows, tiles, side, s):
    G, ksteps = NCU - side, rows // 64
    if s < 1 or ksteps < 16 or (tiles * s) % G:
        return False
    per = -(-ksteps // s)
    if -(-ksteps // per) != s:          # uniir_gemm's split rule would trim s: an empty range
        return False
    return per >= 16 and ksteps - per * (s - 1) >= 16


def test_every_plan_satisfies_the_launch_conditions_and_is_minimal():
    from uniir_amd import _lib
    lib = _lib.load()
    wrong = []
    plans = 0
    for rows in ROWS:
        for tiles in range(1, 601):
            for side in (1, 16, 32, 40, 48, 64, 128, 255):
                s = lib.uniir_gemm_wgrad_side_plan(rows, tiles, side)
                want = next((k for k in range(1, 65) if _ok(rows, tiles, side, k)), 0)
                plans += s > 0
                if s != want or (s and not _ok(rows, tiles, side, s)):
                    wrong.append((rows, tiles, side, s, want))
    assert not wrong, wrong[:10]
    assert plans > 100


def test_the_pairs_of_the_vit_l14_step():
    """263 168 rows: c_fc's gradient (64 tiles) on 224 units is 7 slabs, 2 chunks per workgroup; in_proj's (48 tiles) on 208 units is 13
    slabs, 3 chunks per workgroup"""
    from uniir_amd import _lib
    lib = _lib.load()
    assert lib.uniir_gemm_wgrad_side_plan(263168, 64, 32) == 7 and 64 * 7 == 224 * 2
    assert lib.uniir_gemm_wgrad_side_plan(263168, 48, 48) == 13 and 48 * 13 == 208 * 3


def test_no_side_units_no_plan():
    from uniir_amd import _lib
    lib = _lib.load()
    for side in (0, -1, 256, 300):
        assert lib.uniir_gemm_wgrad_side_plan(263168, 64, side) == 0
    assert lib.uniir_gemm_wgrad_side_plan(263168, 0, 32) == 0
    assert lib.uniir_gemm_wgrad_side_plan(-5, 64, 32) == 0
    assert lib.uniir_gemm_wgrad_ln_bwd(None, *([None] * 1), 0, *([None] * 2), 0, *([None] * 2), 0, *([None] * 5), 0, 0, C.c_float(0), 32,
                                       None) == -1
