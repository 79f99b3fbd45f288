"""CPU tests of the lapse counter and of the scratch registry's locking (include/uniir_hip.h uniir_reduce_stats, uniir_reduce_scratch):
host-side bookkeeping only -- the registered addresses are fake and are never dereferenced, because nothing is launched."""
import ctypes
import os
import re
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reduce_stats_is_exported_declared_and_bound():
    from uniir_amd import _lib, ops
    raw = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(raw, "uniir_reduce_stats"), "uniir_reduce_stats is not exported by libuniir_hip.so"
    header = open(os.path.join(ROOT, "include", "uniir_hip.h")).read()
    assert re.search(r"int\s+uniir_reduce_stats\s*\(\s*int64_t\s*\*\s*fallbacks\s*,\s*int64_t\s*\*\s*max_request\s*,\s*int32_t\s+reset\s*\)\s*;",
                     header), "uniir_reduce_stats(int64_t*, int64_t*, int32_t) is not declared in include/uniir_hip.h"
    assert "uniir_reduce_stats" in _lib.SIGNATURES
    lib = _lib.load()
    f, m = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.uniir_reduce_stats(ctypes.byref(f), ctypes.byref(m), 1) == 0           # read, then reset
    assert f.value >= 0 and m.value >= 0
    assert lib.uniir_reduce_stats(ctypes.byref(f), ctypes.byref(m), 0) == 0
    assert (f.value, m.value) == (0, 0)
    assert lib.uniir_reduce_stats(None, None, 0) == 0                                  # either pointer may be NULL
    assert lib.uniir_reduce_stats(ctypes.byref(f), None, 0) == 0 and lib.uniir_reduce_stats(None, ctypes.byref(m), 0) == 0
    ops.reset_reduce_stats()
    assert ops.reduce_stats() == (0, 0)
    assert lib.uniir_abi_version() >= 4                                                # the library says that it has the entry point


def test_registry_survives_two_threads_registering_at_once():
    """ctypes releases the GIL around every call, so two Python threads really are inside uniir_reduce_scratch at the same time.
    Each works on its own fake stream handle: register, replace, unregister, a few thousand times, while a third thread reads the
    counters.  Every call returns UNIIR_OK, and afterwards both streams can still be registered, replaced and removed."""
    from uniir_amd import _lib
    lib = _lib.load()
    rounds, bad = 4000, []

    def churn(stream, base):
        for i in range(rounds):
            buf = base + 256 * (i % 97)
            rc = (lib.uniir_reduce_scratch(buf, 1 << 20, stream), lib.uniir_reduce_scratch(buf + 256, 2 << 20, stream),
                  lib.uniir_reduce_scratch(None, 0, stream))
            if rc != (0, 0, 0):
                bad.append((stream, i, rc))
                return

    def read():
        f, m = ctypes.c_int64(), ctypes.c_int64()
        for _ in range(rounds):
            if lib.uniir_reduce_stats(ctypes.byref(f), ctypes.byref(m), 0) != 0 or f.value != 0 or m.value != 0:
                bad.append(("stats", f.value, m.value))
                return

    assert lib.uniir_reduce_stats(None, None, 1) == 0
    threads = [threading.Thread(target=churn, args=(0x7001, 0x100000)), threading.Thread(target=churn, args=(0x7002, 0x900000)),
               threading.Thread(target=read)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad, bad[:3]
    for stream in (0x7001, 0x7002):                    # the table is still consistent: each stream registers, replaces and leaves
        assert lib.uniir_reduce_scratch(0x100000, 1 << 20, stream) == 0
        assert lib.uniir_reduce_scratch(0x200000, 2 << 20, stream) == 0
    # ... and a full table (64 slots) still takes new streams by dropping the entry used longest ago
    for k in range(80):
        assert lib.uniir_reduce_scratch(0x300000 + 256 * k, 1 << 20, 0x8000 + k) == 0
    for stream in [0x7001, 0x7002] + [0x8000 + k for k in range(80)]:
        assert lib.uniir_reduce_scratch(None, 0, stream) == 0
    assert lib.uniir_reduce_scratch(0x1001, 1 << 20, 0x7001) == -1                     # validation is unchanged
    f, m = ctypes.c_int64(), ctypes.c_int64()
    assert lib.uniir_reduce_stats(ctypes.byref(f), ctypes.byref(m), 0) == 0 and (f.value, m.value) == (0, 0)   # nothing was launched
