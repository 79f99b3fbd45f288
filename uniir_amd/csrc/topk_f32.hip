// Exact brute-force inner-product top-k over an fp32 candidate pool: the fp32 twin of uniir_topk_ip (topk.hip) for pools that
// were extracted with use_fp16 = False and must rank as the reference's FAISS index over the same fp32 rows does
// (mbeir_retriever.py: the .npy is read with astype("float32"), normalize_L2, IndexFlatIP).  Same contract and the same four
// stages per sweep of queries, every one reading 4-byte rows:
//   norms  : inv_norm_f32_kernel -- the oracle's sequential fp32 sum of squares (no fma), one lane per row, rows fetched by the
//            wave as whole 128-byte lines (the access pattern of inv_norm_kernel);
//   scan   : topk_gmax_f32_kernel -- gmax[q][group of 16 rows] = best APPROXIMATE score, v_mfma_f32_16x16x4_f32 on the operands as
//            they are (no conversion: un-normalised rows of any fp32 magnitude are in range, every product is exact inside the
//            fma, only the fp32 accumulation rounds: topk_select.h tk_slack_cos_f32);
//   select : topk_gsel_f32_kernel -- every group within the proven rounding bound of the k-th best group maximum (GselBound:
//            the rule of the fused fp16 tail, here as a launch of its own);
//   rescore: rescore_f32_kernel -- the oracle's chain (normalise both operands, multiply, add; sequential, contraction off)
//            over the candidate groups' rows, then the type-free sort of topk_tail.hip.
// Which scan was kept and why: the fp32 MFMA runs at about a sixteenth of the fp16 rate, so above ~40 queries per sweep the scan
// is MFMA-bound; a split of every value into two bf16 halves on the 16-bit MFMA would stay HBM-bound
// longer but needs its own bound and range handling -- it is described in experiments/topk/README.md and not built.
#include "topk.h"
#include "topk_select.h"

// ---------------------------------------------------------------------------------------------------------------------------
// inv_norm[i] = 1/sqrt(sum_j x_j^2), sequential fp32 without fma; 0 for a row whose sum is not > 0.  64 rows x 128 B per step, eight
// lanes side by side on a row, through a wave-private LDS slab from which every lane takes its own row's 32 elements.
#define TKF_ROW 144
__global__ __launch_bounds__(256) void inv_norm_f32_kernel(const float* __restrict__ x, long n, int dim, float* __restrict__ inv) {
    __shared__ __attribute__((aligned(16))) char stage[4][64 * TKF_ROW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long row0 = ((long)blockIdx.x * 4 + w) * 64;
    if (row0 >= n) return;                                  // (whole wave; no workgroup barrier below)
    char* st = stage[w];
    const int sub = lane >> 3, ch = lane & 7;
    float s = 0.f;
    for (int c0 = 0; c0 < dim; c0 += 32) {
        const bool live = c0 + ch * 4 < dim;                // the last step of a dim that is not a multiple of 32
        f32x4_t v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const long gr = min(row0 + sub + 8 * i, n - 1);
            v[i] = live ? *reinterpret_cast<const f32x4_t*>(x + gr * dim + c0 + ch * 4) : f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
        __builtin_amdgcn_wave_barrier();                    // the previous step's reads of the slab are done (wave-private, in order)
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4_t*>(st + (sub + 8 * i) * TKF_ROW + ch * 16) = v[i];
        __builtin_amdgcn_wave_barrier();
        const int nch = min(8, (dim - c0) / 4);
        for (int c = 0; c < nch; ++c) {
            const f32x4_t q = *reinterpret_cast<const f32x4_t*>(st + lane * TKF_ROW + c * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __fadd_rn(s, __fmul_rn(q[e], q[e]));
        }
    }
    // 1.0 / sqrtf(s) in double, the f32 sqrt taken through f64 (exactly the correctly rounded f32 result), as inv_norm_kernel
    if (row0 + lane < n) inv[row0 + lane] = s > 0.f ? (float)(1.0 / (double)(float)sqrt((double)s)) : 0.f;
}

extern "C" int uniir_pool_inv_norms_f32(const float* x, int64_t n, int32_t dim, float* inv_norm, void* stream) {
    if (!x || !inv_norm || n < 0 || dim <= 0) return UNIIR_EINVAL;
    if (n == 0) return UNIIR_OK;
    if (dim % 4) return UNIIR_ESHAPE;
    if ((uintptr_t)x & 15) return UNIIR_EALIGN;
    hipLaunchKernelGGL(inv_norm_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (long)n, dim,
                       inv_norm);
    HIP_LAUNCH_CHECK();
    return UNIIR_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The group-max scan.  Workgroup = 4 waves, tile = 128 pool rows x (16 NJ) queries, K in chunks of 32.
//   * Every wave owns 32 pool rows (two MFMA row tiles) against ALL the tile's queries, so its pool rows never pass through LDS:
//     lane (li = lane & 15, lg = lane >> 4) loads 16 bytes of row li at column k0 + 16 h + 4 lg straight into the A operand.
//   * The queries of the chunk are staged once per workgroup in LDS ([16 NJ][32 + 4 pad] floats, double buffered: one barrier per
//     chunk) and read back as 16-byte B operands at the SAME column map, so MFMA e of a 16-column step multiplies element
//     k0 + 16 h + 4 lg + e of the row with element k0 + 16 h + 4 lg + e of the query: a permutation of the summation order,
//     which the bound does not depend on.  Pitch 36 floats: the 16 rows x 16 bytes of a quarter-wave read fall on 64 distinct banks.
//   * D: lane -> query 16 j + li, candidates 4 lg + r of row tile i.  Scaled by the rows' inverse norms, reduced to the group
//     maximum (3 in-lane, 2 cross-lane), parked in LDS and written as one 32-byte run of 8 groups per query.
// Registers (-Rpass-analysis=kernel-resource-usage): 2 x NJ accumulators of 4 + two chunks of A (2 x 16) + one 16-column step of B
// (4 NJ): 206 VGPRs at NJ = 8 (two waves per SIMD, the occupancy planned: 16 independent accumulator tiles per wave cover the
// 40-cycle dependent latency of the 32-cycle MFMA), 112 at NJ = 4 (four waves); no scratch, no spills in any instantiation.
#define TKF_KC 32
#define TKF_PITCH 36
template <int NJ>
__global__ __launch_bounds__(256, 2) void topk_gmax_f32_kernel(const float* __restrict__ pool, const float* __restrict__ pinv,
                                                               long rows, int dim, const float* __restrict__ queries, int nq,
                                                               float* __restrict__ gmax, long ngroups, int tiles_q) {
    constexpr int QB = 16 * NJ;                       // queries per workgroup tile
    constexpr int NB = QB * 8 >= 256 ? QB * 8 / 256 : 1;      // 16-byte pieces of a query chunk per thread (16 queries: 128 pieces)
    __shared__ __attribute__((aligned(16))) float qs[2][QB * TKF_PITCH];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int li = lane & 15, lg = lane >> 4;
    const long ct = blockIdx.x / tiles_q;             // consecutive workgroups share the candidate tile
    const int qt = (int)(blockIdx.x - ct * tiles_q);
    const long m0 = ct * 128 + w * 32;
    const int q0 = qt * QB;
    f32x4_t acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const float* arow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) arow[i] = pool + min(m0 + i * 16 + li, rows - 1) * dim + 4 * lg;      // clamped rows are masked below
    // staging map of the queries: piece p = tid + 256 b -> query p / 8, columns 4 (p % 8) .. + 3 of the chunk
    const float* bsrc[NB];
    bool bok[NB];
    int bdst[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int p = tid + 256 * b, ql = p >> 3, c4 = (p & 7) * 4;
        bok[b] = q0 + ql < nq;
        bsrc[b] = queries + (long)min(q0 + ql, nq - 1) * dim + c4;
        bdst[b] = p < QB * 8 ? ql * TKF_PITCH + c4 : -1;       // -1: a thread beyond the tile's pieces stages nothing
    }
    f32x4_t a[2][2], vb[NB];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) a[i][h] = *reinterpret_cast<const f32x4_t*>(arow[i] + k0 + 16 * h);
#pragma unroll
        for (int b = 0; b < NB; ++b)
            vb[b] = bok[b] ? *reinterpret_cast<const f32x4_t*>(bsrc[b] + k0) : f32x4_t{0.f, 0.f, 0.f, 0.f};
    };
    fetch(0);
#pragma unroll
    for (int b = 0; b < NB; ++b)
        if (bdst[b] >= 0) *reinterpret_cast<f32x4_t*>(&qs[0][bdst[b]]) = vb[b];
    __syncthreads();
    int buf = 0;
    for (int k0 = 0; k0 < dim; k0 += TKF_KC) {
        f32x4_t ac[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int h = 0; h < 2; ++h) ac[i][h] = a[i][h];
        const bool more = k0 + TKF_KC < dim;
        if (more) fetch(k0 + TKF_KC);                          // the next chunk's operands fly while this one is multiplied
        const float* qb = &qs[buf][li * TKF_PITCH + 4 * lg];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4_t bf[NJ];
#pragma unroll
            for (int j = 0; j < NJ; ++j) bf[j] = *reinterpret_cast<const f32x4_t*>(qb + j * 16 * TKF_PITCH + 16 * h);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < NJ; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(ac[i][h][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int b = 0; b < NB; ++b)
                if (bdst[b] >= 0) *reinterpret_cast<f32x4_t*>(&qs[buf ^ 1][bdst[b]]) = vb[b];
        }
        __syncthreads();       // the other buffer is complete; nobody reads this one any more
        buf ^= 1;
    }
    // group maxima -> LDS image [QB queries][8 groups] (the query buffers are idle after the last barrier)
    float* stage = &qs[0][0];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const long r0 = m0 + i * 16 + 4 * lg;
        float iv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) iv[r] = r0 + r < rows ? pinv[r0 + r] : 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float x = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) x = fmaxf(x, r0 + r < rows ? acc[i][j][r] * iv[r] : -INFINITY);
            x = fmaxf(x, __shfl_xor(x, 16, 64));
            x = fmaxf(x, __shfl_xor(x, 32, 64));
            if (lg == 0) stage[(j * 16 + li) * 8 + w * 2 + i] = x;
        }
    }
    __syncthreads();
    for (int p = tid; p < QB * 2; p += 256) {
        const int ql = p >> 1, half = p & 1;
        const int q = q0 + ql;
        const long g0 = ct * 8 + half * 4;
        if (q < nq) {
            float* dst = gmax + (long)q * ngroups + g0;
            const float* src = stage + ql * 8 + half * 4;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                if (g0 + g < ngroups) dst[g] = src[g];
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Candidate groups of a query: gsel_body with the rigorous rule (GselBound) and the fp32 slack; the row indices of the kept groups
// fill a prefix of cand[q][gcap * 16], everything behind them is -1.
template <bool REG>
__global__ __launch_bounds__(1024) void topk_gsel_f32_kernel(const float* __restrict__ gmax, long ngroups, long rows,
                                                             const float* __restrict__ qinv, int dim, int kc, int k, int gcap,
                                                             int* __restrict__ cand) {
    __shared__ float s_iq;
    __shared__ int s_nkept;
    const int q = blockIdx.x;
    GselBound gb;
    gb.k = k;
    gb.slack_cos = tk_slack_cos_f32(dim);
    gb.iq = &s_iq;
    gb.nkept = &s_nkept;
    gsel_body<1024, REG>(gmax + (long)q * ngroups, ngroups, rows, kc, gcap, cand + (long)q * gcap * TK_G,
                         [&] { if (threadIdx.x == 0) s_iq = qinv[q]; }, &gb);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Exact re-score in the contract's order: qn[j] = q[j] * qinv (when qinv != 0), xn[j] = x[j] * pinv (when pinv != 0), both rounded
// to fp32, s = s + qn[j] * xn[j] sequentially, mul then add (this translation unit is built with -ffp-contract=off).  A wave owns
// 64 (query, candidate) pairs; the candidate rows are fetched 128 B at a time by 8 lanes per row, parked in a wave-private LDS
// slab, and each lane then walks ITS row's 32 elements in order (rescore_coalesced_kernel with 4-byte rows).
__global__ __launch_bounds__(256) void rescore_f32_kernel(const float* __restrict__ pool, const float* __restrict__ pinv,
                                                          const float* __restrict__ queries, const float* __restrict__ qinv, int nq,
                                                          int dim, const int* __restrict__ cand_idx, int ncand,
                                                          float* __restrict__ exact) {
    __shared__ __attribute__((aligned(16))) char stage[4][64 * TKF_ROW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long pairs = (long)nq * ncand;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const bool live = t < pairs;
    const int q = live ? (int)(t / ncand) : 0;
    const int ci = live ? cand_idx[t] : -1;
    if (__ballot(ci >= 0) == 0ull) {                        // (wave-uniform) nothing kept in these 64 slots: most of the tail
        if (live) exact[t] = -INFINITY;
        return;
    }
    const float* qr = queries + (long)q * dim;
    const float iq = qinv[q], ic = ci >= 0 ? pinv[ci] : 0.f;
    int rows8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) rows8[i] = __shfl(ci, 8 * i + (lane >> 3), 64);
    const int piece = lane & 7;
    char* mine = &stage[w][0];
    f32x4_t pre[8];
    auto fetch = [&](int c0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const f32x4_t z = {0.f, 0.f, 0.f, 0.f};
            pre[i] = rows8[i] >= 0 ? *reinterpret_cast<const f32x4_t*>(pool + (long)rows8[i] * dim + c0 + piece * 4) : z;
        }
    };
    float s = 0.f;
    fetch(0);
    for (int c0 = 0; c0 < dim; c0 += 32) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *reinterpret_cast<f32x4_t*>(mine + (8 * i + (lane >> 3)) * TKF_ROW + piece * 16) = pre[i];
        __builtin_amdgcn_wave_barrier();
        if (c0 + 32 < dim) fetch(c0 + 32);
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const f32x4_t a = *reinterpret_cast<const f32x4_t*>(qr + c0 + 4 * u);
            const f32x4_t b = *reinterpret_cast<const f32x4_t*>(mine + lane * TKF_ROW + u * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float qa = a[e], ca = b[e];
                if (iq != 0.f) qa = __fmul_rn(qa, iq);
                if (ic != 0.f) ca = __fmul_rn(ca, ic);
                s = __fadd_rn(s, __fmul_rn(qa, ca));
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (live) exact[t] = ci >= 0 ? s : -INFINITY;
}

// ---------------------------------------------------------------------------------------------------------------------------
// uniir_topk_ip_f32: the contract of uniir_topk_ip over fp32 rows.  Workspace: group maxima of one sweep | query inverse norms |
// candidate rows | exact scores.
static int tkf_chunk_max() {
    const int c = tk_sweep_override();
    return c ? c : TK_GPATH_MAXQ;
}
struct TkfLayout { int chunk; int64_t qinv, cand, exact, bytes; };       // sweep width; byte offsets (group maxima at 0); total
static TkfLayout tkf_layout(int32_t nq, int32_t k, int64_t rows) {
    TkfLayout l;
    const int chunk_max = tkf_chunk_max();
    l.chunk = nq < chunk_max ? nq : chunk_max;
    const int64_t cbytes = tk_align256((int64_t)l.chunk * TK_GMULT * (k + 8) * TK_G * 4);
    l.qinv = tk_align256((int64_t)l.chunk * tk_groups(rows) * 4);
    l.cand = l.qinv + tk_align256((int64_t)nq * 4);
    l.exact = l.cand + cbytes;
    l.bytes = l.exact + cbytes + 256;
    return l;
}
extern "C" int64_t uniir_topk_ip_f32_workspace_bytes(int32_t nq, int32_t k, int64_t rows, int32_t dim) {
    if (nq <= 0 || k <= 0 || rows <= 0 || dim <= 0) return 0;
    return tkf_layout(nq, k, rows).bytes;
}

extern "C" int uniir_topk_ip_f32(const float* pool_f32, const float* pool_inv_norm, const int64_t* pool_ids, int64_t rows,
                                 int32_t dim, const float* queries_f32, int32_t nq, int32_t k, float* out_scores,
                                 int64_t* out_ids, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!pool_f32 || !pool_inv_norm || !queries_f32 || !out_scores || !out_ids || !workspace) return UNIIR_EINVAL;
    if (rows <= 0 || nq <= 0 || k <= 0) return UNIIR_EINVAL;
    if (k + 8 > TK_MAXKC || dim % 64 || dim <= 0 || rows > 0x7fffffffL) return UNIIR_ESHAPE;
    // the same cut as the fp16 search: >= 2 GiB of rows is searched as equal sub-shards by the caller (retrieval.subshard_bounds)
    if (!tk_fits31(rows, dim, 4)) return UNIIR_ESHAPE;
    if (((uintptr_t)pool_f32 & 15) || ((uintptr_t)queries_f32 & 15) || ((uintptr_t)pool_inv_norm & 15) || ((uintptr_t)workspace & 255))
        return UNIIR_EALIGN;
    const TkfLayout l = tkf_layout(nq, k, rows);
    if (workspace_bytes < l.bytes) return UNIIR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int chunk = l.chunk;
    const int kc = k + 8, gcap = TK_GMULT * kc, ncand = gcap * TK_G;
    const long ngroups = (long)tk_groups(rows);
    char* ws = (char*)workspace;
    float* gmax = (float*)ws;
    float* qinv = (float*)(ws + l.qinv);
    int32_t* cand = (int32_t*)(ws + l.cand);
    float* exact = (float*)(ws + l.exact);
    int rc = uniir_pool_inv_norms_f32(queries_f32, nq, dim, qinv, stream);
    if (rc) return rc;
    const long tiles_c = (rows + 127) / 128;
    for (int lo = 0; lo < nq; lo += chunk) {
        const int n = nq - lo < chunk ? nq - lo : chunk;
        const float* qp = queries_f32 + (long)lo * dim;
        // the query tile follows the sweep: 16 / 32 / 64 queries (the MFMA work on padding would otherwise put a one-query search on the
        // MFMA roof of 64: measured 0.67 ms at 699 040 rows against the 0.34 ms HBM takes), more: tiles of 128
#define TKF_SCAN(NJ)                                                                                                             \
    hipLaunchKernelGGL((topk_gmax_f32_kernel<NJ>), dim3((unsigned)tiles_c), dim3(256), 0, st, pool_f32, pool_inv_norm, (long)rows, \
                       dim, qp, n, gmax, ngroups, 1)
        if (n <= 16) TKF_SCAN(1);
        else if (n <= 32) TKF_SCAN(2);
        else if (n <= 64) TKF_SCAN(4);
#undef TKF_SCAN
        else {
            const int tiles_q = (n + 127) / 128;
            hipLaunchKernelGGL((topk_gmax_f32_kernel<8>), dim3((unsigned)(tiles_c * tiles_q)), dim3(256), 0, st, pool_f32,
                               pool_inv_norm, (long)rows, dim, qp, n, gmax, ngroups, tiles_q);
        }
        if (tk_sel_reg_ok(rows))
            hipLaunchKernelGGL((topk_gsel_f32_kernel<true>), dim3(n), dim3(1024), 0, st, gmax, ngroups, (long)rows, qinv + lo, dim, kc, k,
                               gcap, cand);
        else
            hipLaunchKernelGGL((topk_gsel_f32_kernel<false>), dim3(n), dim3(1024), 0, st, gmax, ngroups, (long)rows, qinv + lo, dim, kc,
                               k, gcap, cand);
        const long pairs = (long)n * ncand;
        hipLaunchKernelGGL(rescore_f32_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, pool_f32, pool_inv_norm, qp,
                           qinv + lo, n, dim, cand, ncand, exact);
        rc = launch_tail_sort(exact, cand, pool_ids, n, ncand, k, out_scores + (long)lo * k, out_ids + (long)lo * k, st);
        if (rc) return rc;                  // (its launch check covers the sweep's launches)
    }
    return UNIIR_OK;
}
