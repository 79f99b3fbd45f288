"""CPU tests of the C-ABI boundary: libuniir_hip.so loads here (no GPU needed to dlopen) and exports every symbol
that include/uniir_hip.h declares; the ctypes table covers the header; error strings work."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "uniir_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(uniir_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from uniir_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = _header_symbols()
    assert len(syms) >= 30
    for s in syms:
        assert hasattr(lib, s), f"{s} declared in include/uniir_hip.h but not exported"


def test_ctypes_table_matches_header():
    from uniir_amd import _lib
    assert sorted(_lib.SIGNATURES) == _header_symbols()


def test_error_strings_and_version():
    from uniir_amd import _lib
    lib = _lib.load()
    assert lib.uniir_abi_version() >= _lib.ABI_VERSION == 2
    assert lib.uniir_strerror(0) == b"ok"
    assert b"aligned" in lib.uniir_strerror(-3)


def test_product_path_has_no_cpu_fallback():
    import pytest
    import torch
    from uniir_amd import ops
    with pytest.raises(RuntimeError):
        ops.call("uniir_cast_f32_to_bf16", torch.zeros(8), torch.zeros(8, dtype=torch.bfloat16), 8)


def _tower(image=True, layers=24, width=1024, tokens=257, res=224, patch=14):
    from uniir_amd import _lib
    blocks = (_lib.ClipBlock * layers)()
    for b in blocks:
        for name, _ in _lib.ClipBlock._fields_:
            setattr(b, name, 0x1000)            # any non-null address: these calls never touch device memory
    t = _lib.ClipTower()
    t.is_text, t.layers, t.width, t.heads, t.tokens, t.embed_dim = int(not image), layers, width, width // 64, tokens, 768
    t.resolution, t.patch, t.kpad, t.vocab = res, patch, (3 * patch * patch + 63) // 64 * 64, 49408
    t.blocks = ctypes.cast(blocks, ctypes.POINTER(_lib.ClipBlock))
    for name in ("conv16", "class_emb", "pos_emb", "ln_pre_w", "ln_pre_b", "token_emb", "ln_post_w", "ln_post_b", "proj16"):
        setattr(t, name, 0x1000)
    return t, blocks


def test_tower_entry_points_plan_and_validate_on_the_host():
    """[TOWER] uniir_clip_tower_*: the workspace query is pure host arithmetic (ViT-L/14 at the bench batch: the ~190 GB
    activation stash DESIGN.md quotes), malformed descriptions and null pointers are errors, never UB"""
    from uniir_amd import _lib
    lib = _lib.load()
    t, keep = _tower()
    R, W = 1024 * 257, 1024
    need = lib.uniir_clip_tower_workspace_bytes(ctypes.byref(t), 1024, 1)
    per_layer = R * W * (4 + 6 + 2 + 4 + 8 + 2 + 2) + 1024 * 16 * 257 * 4        # x qkv ao x2 f h1 h2 + lse
    assert 24 * per_layer < need < 24 * per_layer * 1.12
    fwd_only = lib.uniir_clip_tower_workspace_bytes(ctypes.byref(t), 1024, 0)
    assert 0 < fwd_only < need / 8                                                # one layer's buffers instead of 24
    assert lib.uniir_clip_tower_workspace_bytes(ctypes.byref(t), 0, 1) > 0
    t.tokens = 256                                                                # != 1 + (224/14)^2
    assert lib.uniir_clip_tower_workspace_bytes(ctypes.byref(t), 8, 1) == -1
    t.tokens, t.width = 257, 1000                                                 # not 64 * heads
    assert lib.uniir_clip_tower_workspace_bytes(ctypes.byref(t), 8, 1) == -1
    t.width = 1024
    assert lib.uniir_clip_tower_fwd(ctypes.byref(t), None, 8, None, None, 0, 1, None) == -1          # UNIIR_EINVAL
    assert lib.uniir_clip_tower_fwd(ctypes.byref(t), 0x1000, 8, 0x1000, 0x1001, 1 << 40, 1, None) == -3   # unaligned workspace
    assert lib.uniir_clip_tower_fwd(ctypes.byref(t), 0x1000, 8, 0x1000, 0x1000, 16, 1, None) == -1   # workspace too small
    assert lib.uniir_clip_tower_bwd_blocks(ctypes.byref(t), 8, 5, 3, 0x1000, 1 << 40, None) == -1    # lo > hi
    tt, keep2 = _tower(image=False, layers=12, width=768, tokens=77)
    assert lib.uniir_clip_tower_workspace_bytes(ctypes.byref(tt), 1024, 1) > 12 * 1024 * 77 * 768 * 28
    tt.token_emb = None
    assert lib.uniir_clip_tower_workspace_bytes(ctypes.byref(tt), 8, 1) == -1
    assert lib.uniir_topk_ip_workspace_bytes(100000, 10, 700000) > 1024 * 43750 * 4
    assert lib.uniir_topk_ip(None, None, None, 10, 64, None, 1, 10, None, None, None, 0, None) == -1


def test_search_host_logic_sweep_size_and_workspace_sizes():
    """host-side decisions of the shard search and of the split-K fp32 product (no device work): the automatic sweep size
    (256 queries where the streaming scans apply: dim 768, >= 2048 groups of 16 rows, a shard under 2 GiB; else 1024), the
    explicit override, workspace sizes that cover either choice, argument validation"""
    from uniir_amd import _lib
    lib = _lib.load()
    assert lib.uniir_topk_set_chunk(0) == 0
    assert lib.uniir_topk_ip_sweep_queries(768, 700_000) == 256
    assert lib.uniir_topk_ip_sweep_queries(768, 32_768) == 256 and lib.uniir_topk_ip_sweep_queries(768, 32_752) == 1024
    assert lib.uniir_topk_ip_sweep_queries(768, 1_398_101) == 256 and lib.uniir_topk_ip_sweep_queries(768, 1_398_102) == 1024
    assert lib.uniir_topk_ip_sweep_queries(512, 700_000) == 1024
    try:
        assert lib.uniir_topk_set_chunk(64) == 0 and lib.uniir_topk_ip_sweep_queries(768, 700_000) == 64
        w64 = lib.uniir_topk_ip_workspace_bytes(1000, 10, 700_000)
        assert lib.uniir_topk_set_chunk(1025) < 0 and lib.uniir_topk_set_chunk(-1) < 0        # rejected, setting unchanged
        assert lib.uniir_topk_ip_sweep_queries(768, 700_000) == 64
    finally:
        assert lib.uniir_topk_set_chunk(0) == 0
    auto = lib.uniir_topk_ip_workspace_bytes(1000, 10, 700_000)
    assert auto > w64 > 0                               # automatic: sized for the larger of the 256- and 1024-query layouts
    assert lib.uniir_topk_ip_workspace_bytes(0, 10, 700_000) == 0 and lib.uniir_topk_ip_workspace_bytes(10, 0, 700_000) == 0
    # split-K fp32 product: b = 256, E = 768 -> 12 output tiles -> 86 slices of the 57 344-long reduction
    assert lib.uniir_sgemm_splitk_workspace_bytes(256, 768, 57_344) == 86 * 256 * 768 * 4
    assert lib.uniir_sgemm_splitk_workspace_bytes(256, 768, 64) == 256 * 768 * 4          # nothing to split: one slab
    assert lib.uniir_sgemm_splitk_workspace_bytes(0, 768, 64) == 0
    assert lib.uniir_sgemm_splitk(None, 1, 1, None, 1, 1, None, 1, 4, 4, 16, 1.0, 0, None, 0, None) < 0
    assert lib.uniir_topk_ip(None, None, None, 10, 768, None, 1, 10, None, None, None, 0, None) < 0


def test_gemm_sampling_rule_never_returns_an_empty_set():
    """uniir_gemm_timing_filter = the rule uniir_gemm_timing_read_ex applies to the sampled launches (timing_filter.h), on plain
    numbers.  Round 5's driver GPU record went red on exactly the first case below: a millisecond-long step whose samples ALL sit
    inside the other stream's merged windows returned zero launches (roofline.achieved null)."""
    from uniir_amd import ops
    # (1) tiny configuration: both towers busy for the whole 4-ms region -> every sample shared -> fall back to all, flagged
    windows = [(0.05 * i, 0.05 * i + 0.04) for i in range(80)]                 # 4 ms of back-to-back text-tower GEMMs
    samples = [(0.4 * i + 0.01, 0.03) for i in range(10)]
    keep, fb = ops.gemm_timing_filter(windows, samples)
    assert fb is True and all(keep) and len(keep) == 10
    # (2) headline shape: 1.3-ms samples, the text tower busy during 15 % of the step -> those samples go, the rest stay, no fallback
    windows = [(100.0 + 0.3 * i, 100.0 + 0.3 * i + 0.25) for i in range(200)]   # 100 .. 160 ms, gaps 0.05 ms
    samples = [(10.0 * i, 1.3) for i in range(40)]                              # 0, 10, .. 390 ms
    keep, fb = ops.gemm_timing_filter(windows, samples)
    assert fb is False
    assert [i for i, k in enumerate(keep) if not k] == [10, 11, 12, 13, 14, 15]          # the samples that begin inside 100 .. 160 ms
    # (3) the gap follows the samples' own duration: two windows 1 ms apart are ONE window for 1.3-ms samples (gap 2.6 ms) and TWO
    #     for 0.1-ms samples (gap 0.2 ms); a sample sitting between them is left out in the first case only
    windows = [(10.0, 11.0), (12.0, 13.0)]
    long_s = [(11.2, 0.5)] + [(100.0 + 5 * i, 1.3 + 0.01 * i) for i in range(20)]
    short_s = [(11.2, 0.5)] + [(100.0 + 5 * i, 0.1) for i in range(20)]
    assert ops.gemm_timing_filter(windows, long_s)[0][0] is False
    assert ops.gemm_timing_filter(windows, short_s)[0][0] is True
    assert ops.gemm_timing_filter(windows, long_s, merge_ms=0.0)[0][0] is True          # an explicit gap overrides the automatic one
    # (4) the automatic gap is capped at 3 ms however long the samples are
    windows = [(10.0, 11.0), (15.0, 16.0)]
    s = [(12.5, 0.5)] + [(100.0 + 50 * i, 20.0) for i in range(20)]
    assert ops.gemm_timing_filter(windows, s)[0][0] is True
    # (5) no windows / no samples / unsorted windows
    assert ops.gemm_timing_filter([], [(0.0, 1.0)]) == ([True], False)
    assert ops.gemm_timing_filter([(0.0, 1.0)], []) == ([], False)
    keep, fb = ops.gemm_timing_filter([(50.0, 51.0), (0.0, 1.0)], [(0.5, 0.1)] + [(10.0 + i, 0.1) for i in range(9)])
    assert keep[0] is False and all(keep[1:]) and fb is False
    # (6) fewer than 8 samples taken, one survives: not a statistic -> all kept
    keep, fb = ops.gemm_timing_filter([(0.0, 10.0)], [(1.0, 0.1), (2.0, 0.1), (20.0, 0.1)])
    assert fb is True and all(keep)


def test_reduce_scratch_registry_validates_its_arguments():
    """uniir_reduce_scratch is host-side bookkeeping (no device call): a 256-byte aligned buffer of positive size per stream;
    NULL removes the entry and is harmless when there is none"""
    from uniir_amd import _lib
    lib = _lib.load()
    assert lib.uniir_reduce_scratch(None, 0, None) == 0
    assert lib.uniir_reduce_scratch(0x1001, 1 << 20, None) == -1           # unaligned
    assert lib.uniir_reduce_scratch(0x1000, 0, None) == -1                 # no size
    assert lib.uniir_reduce_scratch(0x10000, 1 << 20, 0x42) == 0
    assert lib.uniir_reduce_scratch(0x20000, 2 << 20, 0x42) == 0           # re-registration replaces
    assert lib.uniir_reduce_scratch(None, 0, 0x42) == 0


def test_tower_workspace_query_sees_the_pooled_last_block_flag():
    """uniir_clip_tower.pool_last_block is part of the workspace layout (csrc/tower.hip plan()): with it the query adds the [batch]-row
    buffers of the pooled last block -- 9 forward buffers, 6 more with save_for_backward -- and nothing else.  Host arithmetic; also
    pins the ctypes mirror of the struct's last fields (a shifted field would turn the sizes into garbage)."""
    from uniir_amd import _lib
    lib = _lib.load()
    al = lambda x: (x + 255) & ~255
    for image in (True, False):
        t, blocks = _tower(image=image, layers=24 if image else 12, width=1024 if image else 768, tokens=257 if image else 77)
        M, W, H = 1024, t.width, t.heads
        fwd = [M * W * 2, M * W * 2, M * W * 4, M * W * 2, M * H * 4, M * W * 4, M * W * 2, M * 4 * W * 2, M * 4 * W * 2]
        bwd = [M * W * 2, M * 4 * W * 2, M * W * 2, M * W * 4, M * 3 * W * 2, M * W * 2]
        for save in (0, 1):
            t.pool_last_block = 0
            base = lib.uniir_clip_tower_workspace_bytes(ctypes.byref(t), M, save)
            t.pool_last_block = 1
            pooled = lib.uniir_clip_tower_workspace_bytes(ctypes.byref(t), M, save)
            assert base > 0 and pooled - base == sum(al(x) for x in fwd + (bwd if save else [])), (image, save, pooled - base)
        t.stash_act, t.pool_last_block = 1, 1            # the two layout flags are independent
        assert lib.uniir_clip_tower_workspace_bytes(ctypes.byref(t), M, 1) > pooled


# uniir_gemm's descriptor validation (csrc/gemm.hip gemm_check) runs before the library touches the HIP runtime: every malformed
# descriptor below is rejected here, on a machine without a GPU, with its own code.  The addresses are never dereferenced.
_OK_GEMM = dict(A=0x10000, B=0x20000, C=0x30000, M=256, N=128, K=128, lda=128, ldb=128, ldc=128, epilogue=0, k_splits=1, alpha=1.0)
_HT = dict(epilogue=5, a_tmaj=1, b_tmaj=1, lda=256, K=1100)          # the head + tail shape
_GEMM_REJECTS = [
    # (what, changes, expected code name)
    ("null A", dict(A=None), "EINVAL"),
    ("null B", dict(B=None), "EINVAL"),
    ("null C", dict(C=None), "EINVAL"),
    ("M = 0", dict(M=0), "EINVAL"),
    ("N < 0", dict(N=-8), "EINVAL"),
    ("K = 0", dict(K=0), "EINVAL"),
    ("k_splits = 0", dict(k_splits=0), "EINVAL"),
    ("bad epilogue", dict(epilogue=7), "EINVAL"),
    ("split-K without ATOMIC_F32", dict(k_splits=2, epilogue=4), "EINVAL"),
    ("ACT_ONLY with C2", dict(epilogue=6, C2=0x40000), "EINVAL"),
    ("row_scale with F32", dict(epilogue=4, row_scale=0x50000), "EINVAL"),
    ("row_scale with BF16", dict(row_scale=0x50000), "EINVAL"),
    ("BIAS_ACT without C2", dict(epilogue=1), "EINVAL"),
    ("DACT without aux", dict(epilogue=3, ldaux=128), "EINVAL"),
    ("colsum with BF16", dict(colsum=0x60000), "EUNSUPPORTED"),
    ("colsum with BIAS_ACT", dict(epilogue=1, C2=0x40000, colsum=0x60000), "EUNSUPPORTED"),
    ("colsum with ATOMIC_F32", dict(epilogue=5, colsum=0x60000), "EUNSUPPORTED"),
    ("colsum with ACT_ONLY", dict(epilogue=6, colsum=0x60000), "EUNSUPPORTED"),
    ("fp16 DACT", dict(dtype=1, epilogue=3, aux=0x70000, ldaux=128), "EUNSUPPORTED"),
    ("fp16 RESID_F32 with C2", dict(dtype=1, epilogue=2, C2=0x40000), "EUNSUPPORTED"),
    ("N % 8", dict(N=132, ldc=132), "ESHAPE"),
    ("K % 8, K-major A", dict(K=100, b_tmaj=1, ldb=128), "ESHAPE"),
    ("K % 8, K-major B", dict(K=100, a_tmaj=1, lda=256), "ESHAPE"),
    ("M % 8, T-major A", dict(M=252, a_tmaj=1, b_tmaj=1, lda=256, K=100), "ESHAPE"),
    ("lda % 8", dict(lda=132), "EALIGN"),
    ("ldb % 8", dict(ldb=132), "EALIGN"),
    ("ldc % 4", dict(ldc=130), "EALIGN"),
    ("A not 16-B aligned", dict(A=0x10008), "EALIGN"),
    ("B not 16-B aligned", dict(B=0x20008), "EALIGN"),
    ("C not 16-B aligned", dict(C=0x30004), "EALIGN"),
    ("aux not 8-B aligned", dict(epilogue=3, aux=0x70004, ldaux=128), "EALIGN"),
    ("ldaux % 4", dict(epilogue=3, aux=0x70000, ldaux=130), "EALIGN"),
    ("bias not 16-B aligned", dict(bias=0x80008), "EALIGN"),
    ("a_rowsum without a_tmaj", dict(epilogue=5, a_rowsum=0x90000), "EUNSUPPORTED"),
    ("a_rowsum with fp16", dict(epilogue=5, a_tmaj=1, b_tmaj=1, lda=256, ldb=128, dtype=1, a_rowsum=0x90000), "EUNSUPPORTED"),
    ("bad dtype", dict(dtype=2), "EINVAL"),
    # bias with ATOMIC_F32: one meaning on every path or none -- rejected, whatever path the shape would take
    ("bias with ATOMIC_F32, 128-tile shape", dict(epilogue=5, bias=0x80000, K=72), "EUNSUPPORTED"),
    ("bias with ATOMIC_F32, 256-tile shape", dict(epilogue=5, bias=0x80000, K=192), "EUNSUPPORTED"),
    ("bias with ATOMIC_F32, split-K", dict(epilogue=5, bias=0x80000, K=1024, k_splits=4), "EUNSUPPORTED"),
    ("bias with ATOMIC_F32, head + tail", dict(epilogue=5, bias=0x80000, a_tmaj=1, b_tmaj=1, lda=256, K=1100), "EUNSUPPORTED"),
    ("epilogue < 0", dict(epilogue=-1), "EINVAL"),
    # the late refusals (128-tile problems: K % 64, M < 256 or N < 128): after every check above, before anything is launched
    ("colsum with F32, K % 64", dict(epilogue=4, colsum=0x60000, K=72), "EUNSUPPORTED"),
    ("colsum with RESID_F32, M < 256", dict(epilogue=2, colsum=0x60000, M=128), "EUNSUPPORTED"),
    ("colsum with F32, N < 128", dict(epilogue=4, colsum=0x60000, N=64, ldc=64), "EUNSUPPORTED"),
    ("colsum with DACT, 128-tile, ldc % 8", dict(epilogue=3, aux=0x70000, ldaux=128, colsum=0x60000, K=72, ldc=132), "EUNSUPPORTED"),
    ("DACT with C2, 128-tile, ldaux != N", dict(epilogue=3, aux=0x70000, ldaux=136, C2=0x40000, K=72), "EUNSUPPORTED"),
    ("bad dtype, split-K", dict(dtype=2, epilogue=5, K=1024, k_splits=4), "EINVAL"),
    # two neighbouring checks failing together: the earlier one answers (the pairs no descriptor can fail together -- BIAS_ACT
    # without C2 and DACT without aux, DACT without aux and colsum, colsum and the fp16 epilogues -- have no row)
    ("null A and M = 0", dict(A=None, M=0), "EINVAL"),
    ("K = 0 and bad epilogue", dict(K=0, epilogue=7), "EINVAL"),
    ("bad epilogue and split-K", dict(epilogue=7, k_splits=2), "EINVAL"),
    ("split-K ACT_ONLY with C2", dict(k_splits=2, epilogue=6, C2=0x40000), "EINVAL"),
    ("ACT_ONLY with C2 and row_scale", dict(epilogue=6, C2=0x40000, row_scale=0x50000), "EINVAL"),
    ("BIAS_ACT with row_scale, without C2", dict(epilogue=1, row_scale=0x50000), "EINVAL"),
    ("fp16 DACT and N % 8", dict(dtype=1, epilogue=3, aux=0x70000, ldaux=132, N=132, ldc=132), "EUNSUPPORTED"),
    ("N % 8 and K % 8, K-major A", dict(N=132, ldc=132, K=100, b_tmaj=1, ldb=128), "ESHAPE"),
    ("K % 8, K-major A and B", dict(K=100), "ESHAPE"),
    ("K % 8, K-major B and M % 8, T-major A", dict(K=100, M=252, a_tmaj=1, lda=256), "ESHAPE"),
    ("M % 8, T-major A and lda % 8", dict(M=252, a_tmaj=1, lda=260), "ESHAPE"),
    ("lda % 8 and A not 16-B aligned", dict(lda=132, A=0x10008), "EALIGN"),
    ("C and aux not aligned", dict(C=0x30004, epilogue=3, aux=0x70004, ldaux=128), "EALIGN"),
    ("ldaux % 4 and bias not 16-B aligned", dict(epilogue=3, aux=0x70000, ldaux=130, bias=0x80008), "EALIGN"),
    ("bias not 16-B aligned with ATOMIC_F32", dict(epilogue=5, bias=0x80008), "EALIGN"),
    ("bias with ATOMIC_F32 and a_rowsum without a_tmaj", dict(epilogue=5, bias=0x80000, a_rowsum=0x90000), "EUNSUPPORTED"),
    ("a_rowsum without a_tmaj and colsum with F32, 128-tile", dict(epilogue=4, a_rowsum=0x90000, colsum=0x60000, K=72), "EUNSUPPORTED"),
    ("colsum with F32, 128-tile, and ldc % 8", dict(epilogue=4, colsum=0x60000, K=72, ldc=132), "EUNSUPPORTED"),
    ("colsum with DACT, 128-tile, ldc % 8 and C2 with ldaux != N",
     dict(epilogue=3, aux=0x70000, ldaux=136, C2=0x40000, colsum=0x60000, K=72, ldc=132), "EUNSUPPORTED"),
    ("DACT with C2, 128-tile, ldaux != N and bad dtype", dict(dtype=2, epilogue=3, aux=0x70000, ldaux=136, C2=0x40000, K=72), "EUNSUPPORTED"),
    # a late refusal against an early one of another code, and the dtype check (the last of all) against the others
    ("colsum with F32, 128-tile, and ldc % 4", dict(epilogue=4, colsum=0x60000, K=72, ldc=130), "EALIGN"),
    ("a_rowsum with a bad dtype", dict(epilogue=5, a_tmaj=1, b_tmaj=1, lda=256, dtype=2, a_rowsum=0x90000), "EUNSUPPORTED"),
    ("bad dtype and N % 8", dict(dtype=2, N=132, ldc=132), "ESHAPE"),
    ("bad dtype and colsum with F32, 128-tile", dict(dtype=2, epilogue=4, colsum=0x60000, K=72), "EUNSUPPORTED"),
    # the head + tail shape (ATOMIC_F32, both operands T-major, K % 64, K >= 1024): every refusal comes before the head is launched
    ("head + tail, k_splits = 0", dict(_HT, k_splits=0), "EINVAL"),
    ("head + tail, colsum", dict(_HT, colsum=0x60000), "EUNSUPPORTED"),
    ("head + tail, M % 8", dict(_HT, M=260, lda=264), "ESHAPE"),
    ("head + tail, lda % 8", dict(_HT, lda=260), "EALIGN"),
    ("head + tail, C not 16-B aligned", dict(_HT, C=0x30004), "EALIGN"),
    ("head + tail, a_rowsum with fp16", dict(_HT, dtype=1, a_rowsum=0x90000), "EUNSUPPORTED"),
    ("head + tail, a_rowsum with a bad dtype", dict(_HT, dtype=2, a_rowsum=0x90000), "EUNSUPPORTED"),
    ("head + tail, bad dtype", dict(_HT, dtype=2), "EINVAL"),
    ("head + tail, bad dtype, split-K", dict(_HT, dtype=2, k_splits=4), "EINVAL"),
]


def _wgrad_splits_oracle(rows, tiles, n_cu=256):
    """the split-K rule as ops.wgrad_splits stated it before the library exported it: tiles * splits just under a multiple of the 256
    compute units, every split keeping >= 16 K steps of 64 rows"""
    max_s = max(1, rows // (64 * 16))
    best, best_eff = 1, 0.0
    for s in range(1, min(max_s, 64) + 1):
        blocks = tiles * s
        rounds = -(-blocks // n_cu)
        eff = blocks / (rounds * n_cu)
        if blocks >= 0.9 * n_cu and eff >= 0.9:
            return s
        if eff > best_eff + 1e-9:
            best, best_eff = s, eff
    return best


def test_wgrad_splits_of_the_library_equal_the_rule_everywhere():
    """uniir_gemm_wgrad_splits is the one body of the heuristic (ops.wgrad_splits and the C towers call it): equal to the oracle above
    for every row count around its thresholds and 1 .. 600 output tiles"""
    from uniir_amd import _lib, ops
    lib = _lib.load()
    wrong = [(rows, tiles) for rows in (1, 63, 1023, 1024, 1025, 4096, 33280, 35000, 263168, 590848) for tiles in range(1, 601)
             if not lib.uniir_gemm_wgrad_splits(rows, tiles) == ops.wgrad_splits(rows, tiles) == _wgrad_splits_oracle(rows, tiles)]
    assert not wrong, wrong[:10]


def test_gemm_rejects_malformed_descriptors_before_touching_the_device():
    from uniir_amd import _lib
    lib = _lib.load()
    codes = {"EINVAL": -1, "ESHAPE": -2, "EALIGN": -3, "EUNSUPPORTED": -5}
    assert lib.uniir_gemm(None, None) == codes["EINVAL"]
    got = []
    for what, changes, want in _GEMM_REJECTS:
        d = _lib.GemmDesc()
        for k, v in {**_OK_GEMM, **changes}.items():
            setattr(d, k, v)
        got.append((what, lib.uniir_gemm(ctypes.byref(d), None), codes[want]))
    wrong = [g for g in got if g[1] != g[2]]
    assert not wrong, wrong
