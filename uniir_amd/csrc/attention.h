// Shared definitions of the attention kernels (attention.hip: the general 16-row-tile kernels; attention_pair.hip: the persistent
// pair-tile kernels for plain self-attention; attention_long.hip: the streaming kernels; attention_one.hip: the one-query backward):
// argument block, LDS tile layout, fragment helpers -- and, at the end, the host layer of all four files and tower.hip: the two
// sequence limits, the prototypes that cross files, the entry points' check helpers, the AttnArgs builders and the launch helper.
#pragma once
#include "common.h"
#include "../../include/uniir_hip.h"
#include <stdlib.h>

// K / V / Q / dO of a head are read by exactly one workgroup: -DUNIIR_ATT_NT=1 stages them with the nt policy (A/B build).
// MEASURED (round 3, same box, interleaved twice): step 634.5 / 635.6 ms plain, 637.7 / 637.2 ms nt -> stays off.
#ifndef UNIIR_ATT_NT
#define UNIIR_ATT_NT 0
#endif
#if UNIIR_ATT_NT
#define ATT_LD(p) __builtin_nontemporal_load(p)
#else
#define ATT_LD(p) (*(p))
#endif
#define ATT_D 64
#define SCALE_LOG2E 0.18033688011112042f  // (1/sqrt(64)) * log2(e)
#define ATT_SCALE 0.125f
#define LN2F 0.6931471805599453f
#define LOG2EF 1.4426950408889634f

#define ATT_DEFER 8.0f      // attn_fwd_kernel: a row's reference maximum moves when a logit exceeds it by more than this (log2 units)

DEVINL int swz_off(int row, int col) {  // byte offset of element (row, col) in a swizzled [rows][64] bf16 tile
    return row * 128 + ((((col >> 3) ^ (row & 7)) << 4) | ((col & 7) << 1));
}

#define ATT_THREADS 512
#define ATT_WAVES (ATT_THREADS / 64)

// legacy staging (A/B switch UNIIR_ATTN_LEGACY_STAGE=1): one slice, loads 4 deep, one HBM round trip per 2048 chunks
template <int NT>
DEVINL void stage_head(char* lds, const unsigned short* __restrict__ src, long ld, int T, int Tp, int tid) {
    const int total = Tp * 8;
    for (int c0 = 0; c0 < total; c0 += 4 * NT) {
        u32x4_t v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * NT + tid;
            const int row = min(c >> 3, T - 1), kc = c & 7;
            v[u] = ATT_LD(reinterpret_cast<const u32x4_t*>(src + (long)row * ld + kc * 8));
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int c = c0 + u * NT + tid;
            const int row = c >> 3, kc = c & 7;
            if (c < total) {
                const u32x4_t z = {0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4_t*>(lds + row * 128 + ((kc ^ (row & 7)) << 4)) = (row < T) ? v[u] : z;
            }
        }
    }
}
// stage rows [0, Tp) of TWO [T][64] bf16 head slices (row stride `ld` elements each) into swizzled LDS, zero padded.
// ALL loads of both slices are issued before the first LDS store (one HBM round trip per staging instead of one per 2048
// chunks and slice -- four at 257 tokens; the PMC anatomy in profiles/r02_attention_pmc.txt shows the waves parked on
// exactly these waits); loads come from clamped (always valid) addresses, the zero-select happens at the LDS store.
// NL = 16-B loads per thread and slice: ceil(Tp * 8 / NT) (<= 8 for Tp <= 512 at 512 threads; the 384-thread backward only
// runs up to 128 tokens).
// `mid` runs between the loads and the LDS stores: independent work (the backward's per-row statistics with their own global
// loads) that then shares the staging's HBM round trip instead of adding one.
template <int NT, int NL, class F>
DEVINL void stage_two_n(char* ldsA, const unsigned short* __restrict__ srcA, long ldA, char* ldsB,
                        const unsigned short* __restrict__ srcB, long ldB, int T, int Tp, int tid, F&& mid) {
    const int total = Tp * 8;
    u32x4_t va[NL], vb[NL];
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int c = u * NT + tid;
        const int row = min(c >> 3, T - 1), kc = c & 7;
        va[u] = ATT_LD(reinterpret_cast<const u32x4_t*>(srcA + (long)row * ldA + kc * 8));
        vb[u] = ATT_LD(reinterpret_cast<const u32x4_t*>(srcB + (long)row * ldB + kc * 8));
    }
    mid();
#pragma unroll
    for (int u = 0; u < NL; ++u) {
        const int c = u * NT + tid;
        const int row = c >> 3, kc = c & 7;
        if (c < total) {
            const u32x4_t z = {0u, 0u, 0u, 0u};
            const int off = row * 128 + ((kc ^ (row & 7)) << 4);
            *reinterpret_cast<u32x4_t*>(ldsA + off) = (row < T) ? va[u] : z;
            *reinterpret_cast<u32x4_t*>(ldsB + off) = (row < T) ? vb[u] : z;
        }
    }
}
template <int NT, class F>
DEVINL void stage_two(char* ldsA, const unsigned short* __restrict__ srcA, long ldA, char* ldsB,
                      const unsigned short* __restrict__ srcB, long ldB, int T, int Tp, int tid, F&& mid) {
    const int nl = (Tp * 8 + NT - 1) / NT;       // wave-uniform
    if (nl <= 2) stage_two_n<NT, 2>(ldsA, srcA, ldA, ldsB, srcB, ldB, T, Tp, tid, mid);
    else if (nl <= 5) stage_two_n<NT, 5>(ldsA, srcA, ldA, ldsB, srcB, ldB, T, Tp, tid, mid);
    else stage_two_n<NT, 8>(ldsA, srcA, ldA, ldsB, srcB, ldB, T, Tp, tid, mid);
}
template <int NT>
DEVINL void stage_two(char* ldsA, const unsigned short* __restrict__ srcA, long ldA, char* ldsB,
                      const unsigned short* __restrict__ srcB, long ldB, int T, int Tp, int tid) {
    stage_two<NT>(ldsA, srcA, ldA, ldsB, srcB, ldB, T, Tp, tid, [] {});
}
// b128 fragment: 8 consecutive d (k-step s) of row r0 + (lane&15)
DEVINL bf16x8_t frag_rows(const char* lds, int r0, int s, int lane) {
    const int row = r0 + (lane & 15), kc = s * 4 + (lane >> 4);
    return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(lds + row * 128 + ((kc ^ (row & 7)) << 4)));
}
// same fragment straight from global (rows >= T read as zero)
DEVINL bf16x8_t frag_rows_global(const unsigned short* __restrict__ src, long ld, int r0, int s, int lane, int T) {
    const int row = r0 + (lane & 15);
    u32x4_t v = {0u, 0u, 0u, 0u};
    if (row < T) v = *reinterpret_cast<const u32x4_t*>(src + (long)row * ld + s * 32 + (lane >> 4) * 8);
    return __builtin_bit_cast(bf16x8_t, v);
}
// transposed fragment for column tile dt (16 cols) over the 32-row block starting at rb:
// lane (i = col = lane&15, g = lane>>4) gets rows {rb+4g+0..3, rb+16+4g+0..3} of column 16*dt + (lane&15)
DEVINL bf16x8_t frag_cols_tr(const char* lds, int rb, int dt, int lane) {
    const int t = lane & 15, g = lane >> 4;
    const int row = rb + 4 * g + (t >> 2), col = 16 * dt + 4 * (t & 3);
    const s16x4_t lo = lds_read_tr16(lds + swz_off(row, col));
    const s16x4_t hi = lds_read_tr16(lds + swz_off(row + 16, col));
    const u32x2_t l2 = __builtin_bit_cast(u32x2_t, lo), h2 = __builtin_bit_cast(u32x2_t, hi);
    const u32x4_t r = {l2[0], l2[1], h2[0], h2[1]};
    return __builtin_bit_cast(bf16x8_t, r);
}
DEVINL bf16x8_t pack8(const f32x4_t a, const f32x4_t b) {
    const u32x4_t r = {pack_bf16x2(a[0], a[1]), pack_bf16x2(a[2], a[3]), pack_bf16x2(b[0], b[1]),
                       pack_bf16x2(b[2], b[3])};
    return __builtin_bit_cast(bf16x8_t, r);
}
DEVINL f32x4_t mfma16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// the fp16 forward (attn_fwd_kernel<.., F16 = true>): the same fragments, the 16 bits read as fp16
template <bool F16>
DEVINL f32x4_t mfma16x(bf16x8_t a, bf16x8_t b, f32x4_t c) {
    if (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
template <bool F16>
DEVINL bf16x8_t pack8x(const f32x4_t a, const f32x4_t b) {
    const u32x4_t r = {pack16x2<F16>(a[0], a[1]), pack16x2<F16>(a[2], a[3]), pack16x2<F16>(b[0], b[1]), pack16x2<F16>(b[2], b[3])};
    return __builtin_bit_cast(bf16x8_t, r);
}
// 16 rows x 64 columns of gradients (lane = row li, registers: column 16 dt + 4 g + r) -> bf16, 64 contiguous bytes per row and
// store: v_permlane16_swap exchanges the 8-byte pieces of column tiles (0,1) / (2,3) between the lane rows g = (0,1) / (2,3), so
// that every lane ends up with 8 consecutive columns starting at 32 p + {0, 16, 8, 24}[g].
template <bool F16 = false>
DEVINL void att_store_tile(const f32x4_t (&acc)[4], float scale, unsigned short* rowp, bool valid, int g) {
    u32x2_t pk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
        const f32x4_t x = acc[dt] * scale;
        pk[dt] = u32x2_t{pack16x2<F16>(x[0], x[1]), pack16x2<F16>(x[2], x[3])};
    }
    const int dstart = ((g & 1) << 4) | ((g & 2) << 2);      // {0, 16, 8, 24}[g]
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const auto x = __builtin_amdgcn_permlane16_swap(pk[2 * p][0], pk[2 * p + 1][0], false, false);
        const auto y = __builtin_amdgcn_permlane16_swap(pk[2 * p][1], pk[2 * p + 1][1], false, false);
        const u32x4_t v = {x[0], y[0], x[1], y[1]};
        if (valid) *reinterpret_cast<u32x4_t*>(rowp + 32 * p + dstart) = v;
    }
}

// Fixed point of the relative-position-bias gradient: 2^-40 per unit, so a (workgroup, bucket) sum holds |x| < 2^23 and resolves
// 9.1e-13 -- finer than the fp32 rounding of any sum above 1.5e-5, and each term is rounded once (round to nearest) where a float
// accumulator rounds at every add.  A term beyond the range saturates (__float2ll_rn), a NaN term counts as 0: dqkv carries the NaN.
#define ATT_DREL_FIX 1099511627776.0f
DEVINL unsigned long long att_drel_fix(float v) { return (unsigned long long)__float2ll_rn(v * ATT_DREL_FIX); }

// Generalised argument block: self-attention on the packed in_proj layout (q|k|v per token, CLIP / BLIP ViT / BERT self)
// and rectangular cross-attention (BLIP MED: Tq text tokens attending to Tk image tokens) share the kernels.
struct AttnArgs {
    const unsigned short* q;      // [batch][Tq] rows, row stride q_ld, head h at column h*64
    const unsigned short* k;      // [batch][Tk] rows, row stride kv_ld
    const unsigned short* v;
    long q_ld, kv_ld;
    unsigned short* out;          // [batch*Tq][out_ld]
    long out_ld;
    float* lse;                   // [batch][H][Tq]
    const int* klen;              // optional [batch]: keys >= klen[m] are masked (BERT padding mask)
    int Tq, Tk, H, causal;
    const unsigned short* dout;   // backward only: [batch*Tq][out_ld]
    unsigned short* dq;           // [batch][Tq] rows, stride dq_ld
    unsigned short* dk;           // [batch][Tk] rows, stride dkv_ld
    unsigned short* dv;
    long dq_ld, dkv_ld;
    // T5-style attention (CLIP_FF fusion stack): logits = scale * q.k + rel_emb[rel_bucket[key - query + Tq - 1]][h]
    float scale;                  // 1/8 for CLIP / BLIP, 1 for T5
    const float* rel_emb;         // optional [buckets][H] fp32
    const int* rel_bucket;        // [Tq + Tk - 1] bucket of every key - query offset
    float* drel;                  // backward, optional: [buckets][H] += d loss / d rel_emb
    float* drel_part;             // backward, optional: [batch][buckets][H] per-workgroup partials of drel (written; the launcher reduces them)
    int nbuckets;
    // attention-probability dropout (BERT attention_probs_dropout_prob, T5 dropout_rate): P V uses P * mask / keep with
    // mask(seed, ((m H + h) Tq + q) Tk + key) (common.h drop_hash); the softmax statistics stay those of the full P
    float drop_p;
    unsigned drop_seed;
    int legacy_stage;             // 1 = one slice at a time, statistics before it (see launch_attn_bwd for when)
    const int* row_off;           // optional [batch + 1]: packed rows -- item m = rows row_off[m] .. row_off[m + 1] - 1 (Tq = Tk = its
                                  // length <= the Tq given, which stays the stride of lse); no relative-position bias
    int row_off_q_only;           // with row_off: only the QUERY side is packed (cross-attention; K / V dense [batch][Tk], klen allowed)
    const int* kv_row_off;        // optional [batch + 1]: the KEY / VALUE side alone is packed (item m = rows kv_row_off[m] ..): the
                                  // pooled-row attention of a packed text tower's last block (tower.hip): one dense query row per item
    int klen_add;                 // added to klen[m] (the EOT index + 1 = the key count of a pooled causal query)
    // the query part of the dropout coordinate ((m H + h) drop_tq + drop_q0 + q) Tk + key: the builders set Tq and 0 (the call's own
    // rows); a one-query call that stands for row drop_q0 of a call with drop_tq queries sets those (uniir_onequery_fwd / _bwd)
    int drop_tq, drop_q0;
#ifdef UNIIR_EXP_BUILD
    unsigned long long* stamps;   // timing build: [64 workgroups][8 waves][8] s_memtime stamps
    int exp;                      // knock-out bits: 1 phase 1 / compute, 2 phase 2, 4 stage A, 8 stage B, 16 stores
#endif
};
#ifdef UNIIR_EXP_BUILD
extern unsigned long long* g_att_stamps;     // defined in attention.hip (uniir_exp_attn_set)
extern int g_att_exp;
#define ATT_STAMP(i)                                                                                          \
    do {                                                                                                      \
        if (a.stamps) {                                                                                       \
            const int wg_ = (int)blockIdx.x - (int)(gridDim.x / 2);                                           \
            if (wg_ >= 0 && wg_ < 64 && (threadIdx.x & 63) == 0)                                              \
                a.stamps[(wg_ * 8 + (threadIdx.x >> 6)) * 8 + (i)] = __builtin_amdgcn_s_memtime();           \
        }                                                                                                     \
    } while (0)
#define ATT_EXP(bit) (a.exp & (bit))
#else
#define ATT_STAMP(i) do {} while (0)
#define ATT_EXP(bit) 0
#endif

// ---------------- the host layer shared by attention.hip, attention_pair.hip, attention_long.hip, attention_one.hip and tower.hip ----------------
#define ATT_SEQ_MAX 512           // a head's K / V (Q / dO) whole in LDS: every kernel of attention.hip and attention_pair.hip
#define ATT_LONG_SEQ_MAX 1024     // the streaming kernels (attention_long.hip) and the one-query backward (attention_one.hip)

// launchers that cross files
int launch_attn_bwd_pair(const AttnArgs& a, int batch, hipStream_t st);      // attention_pair.hip; 1 = shape not taken
// attention_long.hip: plain dense self-attention up to ATT_LONG_SEQ_MAX tokens (one operand streamed through LDS); everything else is UNIIR_ESHAPE
int launch_attn_long_fwd(const AttnArgs& a, int batch, hipStream_t st, bool f16);
int launch_attn_long_bwd(const AttnArgs& a, int batch, hipStream_t st);
// attention_one.hip: the backward of ONE dense query row per (item, head) against 1 .. ATT_LONG_SEQ_MAX dense keys in one pass over K and V
int launch_attn_one_bwd(const AttnArgs& a, int batch, hipStream_t st);
// attention_long.hip: the streaming forward of the general form (attn_xlong_fwd_kernel) for uniir_onequery_fwd above ATT_SEQ_MAX keys
// and for the fp16 general form (f16: uniir_attn_general_fwd_f16 / uniir_onequery_fwd_f16, no dropout)
int launch_attn_xlong_fwd(const AttnArgs& a, int batch, hipStream_t st, bool f16 = false);

// what tower.hip calls (attention.hip).  The forward: row_off = nullptr for dense rows; f16 = the 16-bit tensors are fp16
int attention_fwd_impl(const void* qkv, void* out, float* lse, const int32_t* row_off, int32_t batch, int32_t seq, int32_t heads,
                       int32_t causal, int f16, void* stream);
// one query row per item: the pooled last block
int attention_pooled_fwd_impl(const void* q, const void* k, const void* v, int64_t kv_ld, void* out, float* lse, const int32_t* klen,
                              int32_t klen_add, const int32_t* kv_row_off, int32_t batch, int32_t tk, int32_t heads, int f16,
                              void* stream);
int attention_pooled_bwd_impl(const void* q, const void* k, const void* v, int64_t kv_ld, const void* out, const void* dout,
                              const float* lse, const int32_t* klen, int32_t klen_add, const int32_t* kv_row_off, void* dq,
                              int64_t dq_ld, void* dk, void* dv, int64_t dkv_ld, int32_t batch, int32_t tk, int32_t heads, void* stream);

// the tail of uniir_attention_rel_bwd and _rel_bwd_long (attention.hip): scratch for the bias gradient's partials, `launch`, their sum
int attention_rel_bwd_tail(AttnArgs& a, float* drel, long nparts, int batch, hipStream_t st,
                           int (*launch)(const AttnArgs&, int, hipStream_t));

// The checks of the entry points.  Which of them an entry point makes, and in which order, differs on purpose (DESIGN.md section 3
// has the table; tests/test_attention_refusals_host.py pins it).
template <class... P>
inline bool att_null(const P*... p) { return (!p || ...); }
template <class... P>
inline bool att_misaligned16(const P*... p) { return (((uintptr_t)p | ...) & 15) != 0; }
template <class... L>
inline bool att_ld_not8(L... ld) { return ((ld | ...) & 7) != 0; }          // 16-byte pieces: leading dimensions in multiples of 8 elements
inline bool att_bad_drop(float p) { return p < 0.f || p >= 1.f; }            // a NaN passes (and runs the kernels without dropout) ...
inline bool att_bad_drop_nan(float p) { return !(p >= 0.f && p < 1.f); }     // ... in the older entry points; the _long ones refuse it

// The two layouts of AttnArgs.  Packed [q|k|v] self-attention (in_proj's output), optionally on packed rows (row_off) ...
inline AttnArgs att_args_packed(const void* qkv, const void* out, const float* lse, int seq, int heads, int causal, float scale,
                                const int* row_off = nullptr) {
    const long W = (long)heads * ATT_D;
    AttnArgs a = {};
    a.q = (const unsigned short*)qkv; a.k = a.q + W; a.v = a.q + 2 * W;
    a.q_ld = a.kv_ld = 3 * W;
    a.out = (unsigned short*)const_cast<void*>(out); a.out_ld = W; a.lse = const_cast<float*>(lse);
    a.Tq = a.Tk = seq; a.H = heads; a.causal = causal; a.scale = scale; a.row_off = row_off;
    a.drop_tq = seq;
    return a;
}
inline void att_args_packed_bwd(AttnArgs& a, const void* dout, void* dqkv) {
    const long W = (long)a.H * ATT_D;
    a.dout = (const unsigned short*)dout;
    a.dq = (unsigned short*)dqkv; a.dk = a.dq + W; a.dv = a.dq + 2 * W;
    a.dq_ld = a.dkv_ld = 3 * W;
}
inline void att_args_rel(AttnArgs& a, const float* rel_emb, const int* rel_bucket, int nbuckets) {
    a.rel_emb = rel_emb; a.rel_bucket = rel_bucket; a.nbuckets = nbuckets;
}
// ... and separate Q and K | V (cross-attention, one query row), the default scale
inline AttnArgs att_args_qkv(const void* q, long q_ld, const void* k, const void* v, long kv_ld, const void* out, long out_ld,
                             const float* lse, int tq, int tk, int heads, const int* key_len = nullptr, int causal = 0) {
    AttnArgs a = {};
    a.q = (const unsigned short*)q; a.k = (const unsigned short*)k; a.v = (const unsigned short*)v;
    a.q_ld = q_ld; a.kv_ld = kv_ld;
    a.out = (unsigned short*)const_cast<void*>(out); a.out_ld = out_ld; a.lse = const_cast<float*>(lse); a.klen = key_len;
    a.Tq = tq; a.Tk = tk; a.H = heads; a.causal = causal; a.scale = ATT_SCALE;
    a.drop_tq = tq;
    return a;
}
inline void att_args_qkv_bwd(AttnArgs& a, const void* dout, void* dq, long dq_ld, void* dk, void* dv, long dkv_ld) {
    a.dout = (const unsigned short*)dout;
    a.dq = (unsigned short*)dq; a.dk = (unsigned short*)dk; a.dv = (unsigned short*)dv;
    a.dq_ld = dq_ld; a.dkv_ld = dkv_ld;
}
inline void att_args_q_rows(AttnArgs& a, const int* q_row_off, int q_only) { a.row_off = q_row_off; a.row_off_q_only = q_only; }
inline void att_args_kv_rows(AttnArgs& a, const int* kv_row_off, int klen_add) { a.kv_row_off = kv_row_off; a.klen_add = klen_add; }
inline void att_args_drop(AttnArgs& a, float drop_p, unsigned drop_seed) { a.drop_p = drop_p; a.drop_seed = drop_seed; }
inline void att_args_drop_at(AttnArgs& a, int drop_tq, int drop_q) { a.drop_tq = drop_tq; a.drop_q0 = drop_q; }

// One launch of kernel K.  A kernel with dynamic LDS (max_lds > 0) gets its limit raised to max_lds before its first launch on a
// device: every kernel, i.e. every instantiation of this template, has its own once-per-device flag.
template <auto K, class... A>
inline int att_launch(int max_lds, dim3 grid, dim3 block, int lds, hipStream_t st, const A&... args) {
    static PerDeviceOnce attr;
    if (max_lds > 0 && attr.first()) (void)hipFuncSetAttribute((const void*)K, hipFuncAttributeMaxDynamicSharedMemorySize, max_lds);
    hipLaunchKernelGGL(K, grid, block, lds, st, args...);
    HIP_LAUNCH_CHECK();
    return UNIIR_OK;
}

