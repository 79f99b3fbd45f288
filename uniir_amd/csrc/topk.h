// Shared by topk.hip (scans, selection kernels, the one-call search) and topk_tail.hip (exact re-score, sorts, merges, fused tail).
#pragma once
#include "gemm_core.h"
#include "gemm_core256.h"
#include "gemm_core_pp.h"
#include "../../include/uniir_hip.h"
#include <stdlib.h>
#include <type_traits>

#define TK_QT 128        // queries per block tile (GEMM N)
#define TK_CT 256        // candidates per MFMA tile (GEMM M): pool rows stream through the 256-row LDS-DMA operand
#define TK_CAP 512       // candidate buffer entries per (block, query) (>= 2 * TK_CT)
#define TK_MAXKC 64
#define TK_RANKCAP 1024    // final sort by rank counting up to this many shortlist entries

struct TkEntry { float score; int idx; };

#define TK_G 16              // pool rows per group (one MFMA row tile): the scans keep one maximum per (query, group)
#define TK_GMULT 2            // groups kept per query = TK_GMULT * kc
#define TK_GPATH_MAXQ 1024

// counted wait on the wave's own LDS-DMA / load queue (the streaming scans and the gather rings order themselves with it)
template <int N>
DEVINL void tkr_wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N));
    __builtin_amdgcn_sched_barrier(0);
}

#define TKT_SORTCAP (2 * TK_MAXKC * TK_G)     // slots topk_tail_sort_kernel ranks: 2048 at most (gcap <= 128 groups)

// ---------------------------------------------------------------------------------------------------------------------------
// Host layer shared by topk.hip, topk_tail.hip and topk_f32.hip: the small expressions, the launcher, the plan (DESIGN.md,
// "Top-k host layer", holds the dispatch table the plan implements).
static inline int64_t tk_groups(int64_t rows) { return (rows + TK_G - 1) / TK_G; }
static inline int64_t tk_align256(int64_t x) { return (x + 255) & ~(int64_t)255; }
// a shard's rows are addressed through 31-bit buffer offsets: rows * dim * elem_bytes < 2 GiB
static inline bool tk_fits31(int64_t rows, int32_t dim, int elem_bytes) { return rows * (int64_t)dim * elem_bytes < ((int64_t)1 << 31); }

// One launch of Kernel, the only place that raises a kernel's dynamic-LDS limit: before its first launch on a device (every
// instantiation of this template has its own once-per-device flag; a kernel launched without dynamic LDS never asks).
template <auto Kernel, typename... Args>
static int tk_launch(dim3 grid, dim3 block, int lds_bytes, hipStream_t st, Args... args) {
    static PerDeviceOnce attr_set;
    if (lds_bytes > 0 && attr_set.first()) (void)hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, st, args...);
    HIP_LAUNCH_CHECK();
    return UNIIR_OK;
}

// What one sweep of n queries over one (sub-)shard launches; scan / sel carry the public values UNIIR_TK_SCAN_* / UNIIR_TK_SEL_*.
struct TkSweep {
    int n;              // queries (0: no such sweep)
    int scan;
    int ncu;            // the streaming scans' grid: one workgroup (four waves) per compute unit
    int nw;             // waves whose maxima the scan leaves beside the group maxima (4 ncu), 0: none
    int fused;          // 1: topk_tail_select_rescore_kernel<parts, ..> + topk_tail_sort_kernel; 0: sel, then uniir_topk_rescore
    int parts;          // the fused tail's workgroups per query: 4 | 2 | 1
    int sel;            // the stand-alone selection that fits the scan (what the fused tail replaces)
    int ncand;          // shortlist entries per query
    int64_t wmax_off;   // uniir_topk_ip: the wave maxima lie behind THIS sweep's group maxima (byte offset in the workspace)
};
struct TkRegion { int64_t off, bytes; };          // batched multi search: bytes = the stride between the sub-shards' parts
// The search of one shard below the buffer bound (uniir_topk_ip): full-width sweeps, then at most one narrower one.
struct TkShardPlan {
    int64_t rows;
    int chunk, kc;                                // sweep width, k + 8
    TkSweep full, rem;
    TkRegion gmax, qinv, cand, exact;
    int64_t bytes;                                // uniir_topk_ip_workspace_bytes_ex
};
// The search of one resident shard of any size (uniir_topk_ip_multi): nsub logical sub-shards of `per` rows, the last one shorter.
struct TkPlan {
    int64_t per, last_rows;
    int nsub;
    int batched;                                  // 1: per sweep one scan per sub-shard, then ONE tail, sort and merge launch
    TkShardPlan sub[2];                           // a full sub-shard (the shard itself when nsub == 1) | the last one
    TkSweep full, rem;                            // batched: the sweeps of every sub-shard (wave maxima only where all write them)
    TkRegion gmax, wmax, cand, exact, list_s, list_i;     // batched
    TkRegion inner, all_s, all_i;                 // the per-sub-shard loop: one uniir_topk_ip workspace, k-lists of all queries
    int64_t bytes;                                // uniir_topk_ip_multi_workspace_bytes
};
// topk.hip: pure host arithmetic, no HIP call.  ncu (the device's compute units) decides only ncu / nw of the sweeps.
TkSweep tk_plan_sweep(int64_t rows, int32_t dim, int32_t n, int32_t kc, int ncu);
void tk_plan(int64_t rows, int32_t dim, int32_t nq, int32_t k, int ncu, TkPlan* p);

// Batched tail (round 5, uniir_topk_ip_multi): ONE tail launch + ONE sort launch serve the scans of all sub-shards of a resident pool
// that is larger than the 31-bit buffer bound -- workgroup (query, part, z) works on sub-shard z = rows [z per, min((z + 1) per,
// rows_total)) with its own descriptors (every sub-shard stays below 2 GiB), its own group / wave maxima and candidate regions; the
// sort writes one k-list per (sub-shard, query) and uniir_topk_merge's kernel combines them.  per == 0: a plain single-shard tail.
struct TkMulti {
    long per;          // rows per sub-shard (a multiple of 32)
    long rows_total;
    long g_stride;     // floats between the sub-shards' group-maxima regions  [nq][ngroups of a full sub-shard]
    long w_stride;     // floats between their wave-maxima regions
    long c_stride;     // entries between their cand / exact regions           [nq][gcap * 16]
    long o_stride;     // entries between their output lists                   [nq][k]
};
// topk_tail.hip: the fused tail behind a finished scan (dense gmax [+ wave maxima at wmax when s.nw > 0]): selection + query norm +
// exact re-score | sort.  The plan said s.fused; nothing is decided here.  mu == nullptr: a plain single-shard tail.
int launch_fused_tail(const TkSweep& s, const void* pool_f16, const float* pinv, const int64_t* pool_ids, int64_t rows, int32_t dim,
                      const void* queries_f16, int32_t kc, int32_t k, const float* gmax, const float* wmax, int32_t* cand,
                      float* exact, float* out_scores, int64_t* out_ids, hipStream_t st, const TkMulti* mu = nullptr, int nsub = 1);
// topk_f32.hip (the fp32 twin of the one-call search) shares two host-side pieces with the fp16 search: the explicit sweep width of
// uniir_topk_set_chunk (0 = automatic) and the type-free sort behind an exact re-score (topk_tail_sort_kernel: exact / cand
// [nq][ncand <= 2048] -> the k best by (score desc, id asc), FAISS padding)
int tk_sweep_override();
int launch_tail_sort(const float* exact, const int32_t* cand, const int64_t* pool_ids, int32_t nq, int32_t ncand, int32_t k,
                      float* out_scores, int64_t* out_ids, hipStream_t st);
