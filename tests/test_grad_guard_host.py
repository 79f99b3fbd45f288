"""Host-side checks of the gradient guard that need no device: the library's refusals (all raised before anything is launched), the
workspace formula, the settings (arguments, YAML keys, environment), the optimizer's state_dict, and that a default NativeAdamW holds
no guard at all."""
import ctypes as C

import pytest
import torch

EINVAL, EALIGN = -1, -3


def _lib():
    from uniir_amd import _lib
    return _lib.load()


def _arrays(ptrs, counts):
    n = len(counts)
    return (C.c_void_p * max(1, n))(*ptrs), (C.c_int64 * max(1, n))(*counts), n


def _guard(ptrs, counts, scale=1.0, max_norm=0.0, ctl=0x1000, ws=0x10000, ws_bytes=1 << 20, n=None):
    p, c, k = _arrays(ptrs, counts)
    return _lib().uniir_grad_guard(p, c, k if n is None else n, scale, max_norm, 0, ctl, ws, ws_bytes, None)


def test_chunk_is_a_constant_multiple_of_the_workgroup_tile():
    chunk = _lib().uniir_grad_guard_chunk()
    assert chunk == _lib().uniir_grad_guard_chunk() and chunk >= 1024 and chunk % 1024 == 0


def test_workspace_formula():
    lib = _lib()
    chunk = lib.uniir_grad_guard_chunk()

    def need(*counts):
        _, c, n = _arrays([0] * len(counts), counts)
        return lib.uniir_grad_guard_workspace_bytes(c, n)

    def formula(*counts):          # an fp64 partial and a 64-bit key per chunk, rounded up to 256 bytes
        chunks = sum(-(-c // chunk) for c in counts)
        return -(-chunks * 16 // 256) * 256

    assert need() == 0 and need(0, 0) == 0
    assert need(1) == 256 and need(chunk) == 256 and need(16 * chunk) == 256 and need(16 * chunk + 1) == 512
    for counts in ((1003, chunk + 1, 5), (427_616_513,), (chunk - 1, chunk, chunk + 1, 2 * chunk + 5, 0)):
        assert need(*counts) == formula(*counts)
    assert need(5, -1) == -1 and need(1 << 40) == -1
    assert lib.uniir_grad_guard_workspace_bytes(None, 1) == -1 and lib.uniir_grad_guard_workspace_bytes(None, -1) == -1
    assert lib.uniir_grad_guard_workspace_bytes(None, 0) == 0


def test_guard_refusals_need_no_device():
    nan = float("nan")
    assert _guard([0x2000], [8], ctl=None) == EINVAL                               # NULL control block
    assert _guard([None], [8]) == EINVAL                                           # NULL range
    assert _guard([0x2000], [8], ws=None) == EINVAL                                # NULL workspace that has to hold a partial
    assert _lib().uniir_grad_guard(None, None, 1, 1.0, 0.0, 0, 0x1000, 0x10000, 1 << 20, None) == EINVAL
    assert _guard([0x2000], [-1]) == EINVAL                                        # negative count
    assert _guard([0x2000], [8], n=-1) == EINVAL
    assert _guard([0x2000], [8], scale=nan) == EINVAL and _guard([0x2000], [8], scale=-0.5) == EINVAL
    assert _guard([0x2000], [8], max_norm=nan) == EINVAL
    assert _guard([0x2000], [8], ws_bytes=255) == EINVAL                           # short workspace
    assert _guard([0x2000, 0x3000], [8, 20 * 65536 * 16], ws_bytes=256) == EINVAL
    assert _guard([0x2004], [8]) == EALIGN                                         # range not 16-byte aligned
    assert _guard([0x2000, 0x3008], [8, 8]) == EALIGN
    assert _guard([0x2000], [8], ctl=0x1008) == EALIGN                             # control block
    assert _guard([0x2000], [8], ws=0x10010) == EALIGN                             # workspace: 256 bytes
    # EINVAL is found before EALIGN
    assert _guard([0x2004], [-8]) == EINVAL and _guard([0x2004], [8], scale=nan) == EINVAL


def test_guarded_adamw_refusals_need_no_device():
    lib = _lib()

    def call(p=0x1000, g=0x2000, m=0x3000, v=0x4000, s=0x5000, count=8, step=1, ctl=0x6000):
        return lib.uniir_adamw_step_guarded(p, g, m, v, s, count, 1e-3, 0.9, 0.98, 1e-6, 0.2, step, 1.0, ctl, None)

    assert call(ctl=None) == EINVAL and call(p=None) == EINVAL and call(g=None) == EINVAL
    assert call(count=-1) == EINVAL and call(step=0) == EINVAL
    assert call(ctl=0x6008) == EALIGN and call(m=0x3004) == EALIGN and call(s=0x5002) == EALIGN
    assert call(count=0) == 0 and call(count=0, s=None) == 0                       # nothing to do, nothing launched


def test_control_block_layout():
    from uniir_amd import _lib
    assert C.sizeof(_lib.GradCtl) == 64
    off = {n: getattr(_lib.GradCtl, n).offset for n, _ in _lib.GradCtl._fields_}
    assert off == {"sumsq": 0, "norm": 8, "coef": 12, "nonfinite": 16, "skip": 20, "first_bad_range": 24, "first_bad_chunk": 28,
                   "first_bad_index": 32, "steps_seen": 40, "steps_skipped": 48, "reserved": 56}


# ---- settings ------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def clean_env(monkeypatch):
    monkeypatch.delenv("UNIIR_MAX_GRAD_NORM", raising=False)
    monkeypatch.delenv("UNIIR_SKIP_NONFINITE", raising=False)
    return monkeypatch


def test_settings_from_arguments_yaml_and_environment(clean_env):
    from uniir_amd.trainer import guard_settings
    assert guard_settings() == (None, False)
    assert guard_settings(trainer_config={"learning_rate": 1e-5, "print_freq": 50}) == (None, False)      # a reference YAML
    assert guard_settings(trainer_config={"max_grad_norm": 1.0}) == (1.0, False)
    assert guard_settings(trainer_config={"skip_nonfinite_steps": True}) == (None, True)
    assert guard_settings(trainer_config={"max_grad_norm": "2.5", "skip_nonfinite_steps": True}) == (2.5, True)
    assert guard_settings(trainer_config={"max_grad_norm": 0}) == (None, False)                           # <= 0: no clipping
    assert guard_settings(3.0, True, trainer_config={"max_grad_norm": 1.0}) == (3.0, True)                # an argument wins
    clean_env.setenv("UNIIR_MAX_GRAD_NORM", "0.5")
    clean_env.setenv("UNIIR_SKIP_NONFINITE", "1")
    assert guard_settings() == (0.5, True)
    assert guard_settings(trainer_config={"max_grad_norm": 1.0, "skip_nonfinite_steps": False}) == (1.0, False)   # the YAML wins
    assert guard_settings(2.0) == (2.0, True)
    clean_env.setenv("UNIIR_SKIP_NONFINITE", "0")
    clean_env.setenv("UNIIR_MAX_GRAD_NORM", "")
    assert guard_settings() == (None, False)
    with pytest.raises(ValueError):
        guard_settings(float("nan"))
    clean_env.setenv("UNIIR_MAX_GRAD_NORM", "much")
    with pytest.raises(ValueError):
        guard_settings()


class _Model:
    """what NativeAdamW asks of a model, on the CPU: nothing here reaches a kernel"""

    def __init__(self):
        self.a, self.b = torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(5))

    def optimizer_groups(self):
        return [self.a], [self.b]

    def adamw_group(self, name):
        return 0

    def _ensure_flat(self):
        raise AssertionError("no device work in these tests")


def test_default_optimizer_holds_no_guard(clean_env):
    from uniir_amd.trainer import NativeAdamW
    opt = NativeAdamW(_Model())
    assert opt.guard is None and opt.grad_stats() is None
    sd = opt.state_dict()
    assert sorted(sd) == ["exp_avg", "exp_avg_sq", "extra", "opt_step", "param_groups"]                   # today's checkpoint
    from uniir_amd.host_utils import scaler_state
    assert scaler_state(opt) == {}


def test_environment_switches_build_a_guard(clean_env):
    from uniir_amd.trainer import NativeAdamW
    clean_env.setenv("UNIIR_SKIP_NONFINITE", "1")
    opt = NativeAdamW(_Model())
    assert opt.guard is not None and opt.guard.skip_nonfinite and opt.guard.max_grad_norm is None
    assert opt.guard.ctl is None and opt.guard.workspace is None                                          # nothing allocated yet


def test_state_dict_round_trip_with_and_without_the_keys(clean_env):
    from uniir_amd.host_utils import scaler_state
    from uniir_amd.trainer import NativeAdamW
    opt = NativeAdamW(_Model(), max_grad_norm=1.5, skip_nonfinite=True)
    opt.opt_step = 11
    opt.guard.load_counters(12, 1)
    sd = opt.state_dict()
    assert (sd["steps_seen"], sd["steps_skipped"], sd["max_grad_norm"], sd["skip_nonfinite"], sd["opt_step"]) == (12, 1, 1.5, True, 11)
    assert scaler_state(opt) == {"steps_seen": 12, "steps_skipped": 1}
    twin = NativeAdamW(_Model(), max_grad_norm=0.5)
    twin.load_state_dict(sd)
    assert (twin.opt_step, twin.guard.steps_seen, twin.guard.steps_skipped) == (11, 12, 1)
    assert twin.guard.max_grad_norm == 0.5 and not twin.guard.skip_nonfinite                              # the settings are the run's own
    old = {k: v for k, v in sd.items() if k not in ("steps_seen", "steps_skipped", "max_grad_norm", "skip_nonfinite")}
    twin.load_state_dict(old)                                                                              # a checkpoint from before
    assert (twin.opt_step, twin.guard.steps_seen, twin.guard.steps_skipped) == (11, 0, 0)
    plain = NativeAdamW(_Model())
    plain.load_state_dict(sd)                                                                              # and the other way round
    assert plain.guard is None and plain.opt_step == 11
