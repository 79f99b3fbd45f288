// One-query attention backward (head_dim 64, bf16, scale 1/8): ONE query row per (item, head) against 1 .. ATT_LONG_SEQ_MAX (1024) dense keys, no mask,
// no dropout, no bias.  The pooled last block of a tower (tower.hip: the class token is all that leaves a vision tower) and
// uniir_attention_one_bwd.  (With key counts, packed keys and dropout: uniir_onequery_bwd, see the end of this comment.)
//
// With one query nothing is summed over queries:
//   dV[j] = p_j dO                  rank 1
//   dK[j] = scale dS_j q            rank 1
//   dQ    = scale sum_j dS_j k_j    the only sum
// with p_j = exp2(scale log2e q.k_j - lse log2e), dP_j = dO.v_j, dS_j = p_j (dP_j - delta), delta = dO.O.  So the whole backward is
// ONE pass over K and V: 128 bytes of each read per key and head, 128 bytes of dK and dV written -- a bandwidth-bound kernel in
// the shape of a decode step (GEMV, M = 1): operands go straight to registers as 16-byte pieces, there is no LDS, no barrier and no
// atomic.  (The streaming backward of attention_long.hip at Tq = 1 reads K and V twice in two kernels whose tiles hold one live
// row in 16 and whose workgroups spend 7 waves in 8 on staging alone.)
//
// One wave per (item, head); the AO_WAVES waves of a workgroup take adjacent heads of one item, so a workgroup reads contiguous
// row segments (a wave behind the last head leaves at once: nothing waits for it).  Lane = 8 kk + c: key slot kk (0 .. 7) of a load
// group, 16-byte piece c (columns 8 c .. 8 c + 7) of the 128-byte head row.  A step issues AO_U = 4 loads of K and 4 of V per lane
// (8 keys each: 32 keys per step) before the first use; 104 VGPRs, no scratch, 4 waves per SIMD -- the 4096 waves of 256 items x 16
// heads are resident at once (8 loads per operand: 154 VGPRs, or spills at 128).  A row dot is 8 per-lane products and a fixed butterfly over the row's 8
// neighbouring lanes (the scheme of al_delta), which leaves the sum in all 8.  dQ: every lane adds the keys of its slot in key order
// into 8 fp32 partials; at the end a fixed butterfly over the 8 slots (lane xor 8, 16, 32).  Every sum has one order: two calls give
// the same bits.  Values are rounded to bf16 at the stores of dq / dk / dv only.
// Keys behind tk: their loads are clamped to the last row (always valid), their dS is zero, nothing is stored for them.
//
// The extended form (uniir_onequery_bwd: BLIP's last BERT layer on the class row) is the same body with a per-item key count -- key_len,
// or the item's own packed rows -- and the dropout factor of the full call's coordinates (ao_bwd_body<true, DROP>): the sweep stops at
// the item's key count, the dense rows behind it get exact zeros in dk / dv without being read.  Still no LDS, no atomic, one order
// per sum.  116 VGPRs without and 118 with dropout, no scratch, 4 waves per SIMD like the plain kernel, whose instantiation
// <false, false> is the code above unchanged (104 VGPRs).
#include "attention.h"

#define AO_WAVES 4
#define AO_U 4                       // loads of K (and of V) in flight per lane and step
#define AO_STEP (8 * AO_U)           // keys per step

DEVINL void ao_unpack(float (&f)[8], const u32x4_t v) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        f[2 * e] = __uint_as_float(v[e] << 16);
        f[2 * e + 1] = __uint_as_float(v[e] & 0xffff0000u);
    }
}
DEVINL float ao_dot8(const float (&x)[8], const float (&y)[8]) {
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) s = __builtin_fmaf(x[e], y[e], s);
    return s;
}
// the sum over the 8 lanes of a row, the same in all of them
DEVINL float ao_row_sum(float s) {
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    return s;
}
DEVINL u32x4_t ao_pack(const float (&x)[8], float f) {
    return u32x4_t{pack_bf16x2(x[0] * f, x[1] * f), pack_bf16x2(x[2] * f, x[3] * f), pack_bf16x2(x[4] * f, x[5] * f),
                   pack_bf16x2(x[6] * f, x[7] * f)};
}

// EXT: the extended form (uniir_onequery_bwd).  The item's keys are kvalid = min(Tk, klen[m]) of its Tk dense rows, whose rows kvalid ..
// Tk - 1 get exact zeros in dk / dv, or its own packed rows kv_row_off[m] .. (all of them keys: nothing lies behind them).  DROP: the
// factor f_j of key j, drawn at the coordinate ((m H + h) drop_tq + drop_q0) Tk + j of the call this row stands for, enters where
// the math has it: dV[j] = (p_j f_j) dO, dP_j = f_j (dO . v_j); delta = dO . O already holds it.  <false, false> is the plain kernel.
template <bool EXT, bool DROP>
DEVINL void ao_bwd_body(const AttnArgs& a, int nhb) {
    const int hb = blockIdx.x % nhb, m = blockIdx.x / nhb;
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = hb * AO_WAVES + w;
    if (h >= a.H) return;          // wave-uniform; no barrier follows
    const int kk = lane >> 3, c = lane & 7;
    int Tk = a.Tk;                 // the keys of the sweep
    int nrow = Tk;                 // EXT: the dk / dv rows the item owns
    long kr0 = (long)m * Tk;
    if (EXT) {
        if (a.kv_row_off) {
            kr0 = a.kv_row_off[m];
            nrow = Tk = min(Tk, a.kv_row_off[m + 1] - a.kv_row_off[m]);
        } else if (a.klen) {
            Tk = min(Tk, a.klen[m]);
        }
    }
    const long col = (long)h * ATT_D + c * 8;
    float qf[8], dof[8];
    float delta;
    {
        float of[8];
        ao_unpack(qf, *reinterpret_cast<const u32x4_t*>(a.q + (long)m * a.q_ld + col));
        ao_unpack(dof, *reinterpret_cast<const u32x4_t*>(a.dout + (long)m * a.out_ld + col));
        ao_unpack(of, *reinterpret_cast<const u32x4_t*>(a.out + (long)m * a.out_ld + col));
        delta = ao_row_sum(ao_dot8(dof, of));
    }
    const float lse2 = a.lse[(long)m * a.H + h] * LOG2EF;
    const unsigned short* kp = a.k + kr0 * a.kv_ld + col;
    const unsigned short* vp = a.v + kr0 * a.kv_ld + col;
    unsigned short* dkp = a.dk + kr0 * a.dkv_ld + col;
    unsigned short* dvp = a.dv + kr0 * a.dkv_ld + col;
    const unsigned dth = DROP ? drop_threshold(a.drop_p) : 0u;
    const float dks = DROP ? 1.0f / (1.0f - a.drop_p) : 1.0f;
    const unsigned rowbase = DROP ? (unsigned)((((long)m * a.H + h) * a.drop_tq + a.drop_q0) * a.Tk) : 0u;
    float dq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) dq[e] = 0.f;
    for (int j0 = 0; j0 < Tk; j0 += AO_STEP) {
        u32x4_t rk[AO_U], rv[AO_U];
#pragma unroll
        for (int u = 0; u < AO_U; ++u) {
            const long j = min(j0 + u * 8 + kk, Tk - 1);
            rk[u] = ATT_LD(reinterpret_cast<const u32x4_t*>(kp + j * a.kv_ld));
            rv[u] = ATT_LD(reinterpret_cast<const u32x4_t*>(vp + j * a.kv_ld));
        }
#pragma unroll
        for (int u = 0; u < AO_U; ++u) {
            const int j = j0 + u * 8 + kk;
            float kf[8], vf[8];
            ao_unpack(kf, rk[u]);
            ao_unpack(vf, rv[u]);
            const float s = ao_row_sum(ao_dot8(qf, kf));
            float dp = ao_row_sum(ao_dot8(dof, vf));
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s, SCALE_LOG2E, -lse2));
            const bool live = j < Tk;
            float pv = p;          // what multiplies dO in dV
            if (DROP) {
                const float mk = drop_scale(rowbase + (unsigned)j, a.drop_seed, dth, dks);
                pv = p * mk;
                dp *= mk;
            }
            const float ds = live ? p * (dp - delta) : 0.f;
            if (live) {
                *reinterpret_cast<u32x4_t*>(dvp + (long)j * a.dkv_ld) = ao_pack(dof, pv);
                *reinterpret_cast<u32x4_t*>(dkp + (long)j * a.dkv_ld) = ao_pack(qf, ATT_SCALE * ds);
            } else if (EXT && j < nrow) {          // a masked key inside the last step of the sweep
                const u32x4_t z = {0u, 0u, 0u, 0u};
                *reinterpret_cast<u32x4_t*>(dvp + (long)j * a.dkv_ld) = z;
                *reinterpret_cast<u32x4_t*>(dkp + (long)j * a.dkv_ld) = z;
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) dq[e] = __builtin_fmaf(ds, kf[e], dq[e]);
        }
    }
    if (EXT) {          // the masked keys behind the sweep: exact zeros, nothing is read
        const u32x4_t z = {0u, 0u, 0u, 0u};
        for (int j = (max(Tk, 0) + AO_STEP - 1) / AO_STEP * AO_STEP + kk; j < nrow; j += 8) {
            *reinterpret_cast<u32x4_t*>(dvp + (long)j * a.dkv_ld) = z;
            *reinterpret_cast<u32x4_t*>(dkp + (long)j * a.dkv_ld) = z;
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        dq[e] += __shfl_xor(dq[e], 8);
        dq[e] += __shfl_xor(dq[e], 16);
        dq[e] += __shfl_xor(dq[e], 32);
    }
    if (kk == 0) *reinterpret_cast<u32x4_t*>(a.dq + (long)m * a.dq_ld + col) = ao_pack(dq, ATT_SCALE);
}
__global__ __launch_bounds__(AO_WAVES * 64) void attn_one_bwd_kernel(AttnArgs a, int nhb) { ao_bwd_body<false, false>(a, nhb); }
template <bool DROP>
__global__ __launch_bounds__(AO_WAVES * 64) void attn_onex_bwd_kernel(AttnArgs a, int nhb) { ao_bwd_body<true, DROP>(a, nhb); }

// a: Tq = 1, dense q / out / dout rows [batch][H * 64] (q_ld, out_ld), lse [batch][H], K / V rows [batch * Tk] (kv_ld), dq rows [batch]
// (dq_ld), dk / dv rows [batch * Tk] (dkv_ld); no key counts, no packed rows, no bias, no dropout, the default scale
int launch_attn_one_bwd(const AttnArgs& a, int batch, hipStream_t st) {
    if (a.Tq != 1 || a.Tk < 1 || a.Tk > ATT_LONG_SEQ_MAX || a.causal || a.klen || a.row_off || a.kv_row_off || a.rel_emb ||
        a.drop_p != 0.f || a.scale != ATT_SCALE)
        return UNIIR_ESHAPE;
    if (att_ld_not8(a.q_ld, a.out_ld, a.kv_ld, a.dq_ld, a.dkv_ld)) return UNIIR_EALIGN;      // 16-byte pieces
    if (att_misaligned16(a.q, a.k, a.v, a.out, a.dout, a.dq, a.dk, a.dv)) return UNIIR_EALIGN;
    const int nhb = (a.H + AO_WAVES - 1) / AO_WAVES;
    const long grid = (long)batch * nhb;
    if (grid > 0x7fffffffL) return UNIIR_ESHAPE;
    return att_launch<attn_one_bwd_kernel>(0, dim3((unsigned)grid), dim3(AO_WAVES * 64), 0, st, a, nhb);      // no LDS
}

// the alignment checks are the launcher's: UNIIR_EALIGN for a leading dimension as well
extern "C" int uniir_attention_one_bwd(const void* q, const void* k, const void* v, int64_t kv_ld, const void* out, const void* dout,
                                       const float* lse, void* dq, int64_t dq_ld, void* dk, void* dv, int64_t dkv_ld, int32_t batch,
                                       int32_t tk, int32_t heads, void* stream) {
    if (att_null(q, k, v, out, dout, lse, dq, dk, dv) || batch < 0 || heads <= 0) return UNIIR_EINVAL;
    if (batch == 0) return UNIIR_OK;
    if (tk < 1 || tk > ATT_LONG_SEQ_MAX) return UNIIR_ESHAPE;
    const long W = (long)heads * ATT_D;
    AttnArgs a = att_args_qkv(q, W, k, v, kv_ld, out, W, lse, 1, tk, heads);
    att_args_qkv_bwd(a, dout, dq, dq_ld, dk, dv, dkv_ld);
    return launch_attn_one_bwd(a, batch, (hipStream_t)stream);
}

// ---------------- the extended form: key counts or packed keys, dropout at the coordinates of the full call ----------------
// a: as for launch_attn_one_bwd, with klen OR kv_row_off, drop_p / drop_seed and drop_tq / drop_q0 (att_args_drop_at).  A call without
// any of them is the plain kernel (the same bits by construction: the extended body is that kernel plus these three).
static int launch_attn_onex_bwd(const AttnArgs& a, int batch, hipStream_t st) {
    if (a.Tq != 1 || a.Tk < 1 || a.Tk > ATT_LONG_SEQ_MAX || a.causal || a.row_off || a.rel_emb || (a.klen && a.kv_row_off) || a.klen_add ||
        a.scale != ATT_SCALE)
        return UNIIR_ESHAPE;
    const int nhb = (a.H + AO_WAVES - 1) / AO_WAVES;
    const long grid = (long)batch * nhb;
    if (grid > 0x7fffffffL) return UNIIR_ESHAPE;
    const dim3 g((unsigned)grid), b(AO_WAVES * 64);
    const bool drop = a.drop_p > 0.f;
    if (!a.klen && !a.kv_row_off && !drop) return att_launch<attn_one_bwd_kernel>(0, g, b, 0, st, a, nhb);
    if (!drop) return att_launch<attn_onex_bwd_kernel<false>>(0, g, b, 0, st, a, nhb);
    return att_launch<attn_onex_bwd_kernel<true>>(0, g, b, 0, st, a, nhb);
}
extern "C" int uniir_onequery_bwd(const void* q, int64_t q_ld, const void* k, const void* v, int64_t kv_ld, const void* out,
                                  const void* dout, int64_t out_ld, const float* lse, const int32_t* key_len, const int32_t* kv_row_off,
                                  void* dq, int64_t dq_ld, void* dk, void* dv, int64_t dkv_ld, int32_t batch, int32_t tk, int32_t heads,
                                  float drop_p, uint32_t drop_seed, int32_t drop_tq, int32_t drop_q, void* stream) {
    if (att_null(q, k, v, out, dout, lse, dq, dk, dv) || batch < 0 || heads <= 0) return UNIIR_EINVAL;
    if (att_bad_drop_nan(drop_p) || drop_tq < 1 || drop_q < 0 || drop_q >= drop_tq || (key_len && kv_row_off)) return UNIIR_EINVAL;
    if (batch == 0) return UNIIR_OK;
    if (tk < 1 || tk > ATT_LONG_SEQ_MAX) return UNIIR_ESHAPE;
    if (att_ld_not8(q_ld, kv_ld, out_ld, dq_ld, dkv_ld)) return UNIIR_EALIGN;
    if (att_misaligned16(q, k, v, out, dout, dq, dk, dv)) return UNIIR_EALIGN;
    AttnArgs a = att_args_qkv(q, q_ld, k, v, kv_ld, out, out_ld, lse, 1, tk, heads, key_len);
    att_args_kv_rows(a, kv_row_off, 0);
    att_args_qkv_bwd(a, dout, dq, dq_ld, dk, dv, dkv_ld);
    att_args_drop(a, drop_p, drop_seed);
    att_args_drop_at(a, drop_tq, drop_q);
    return launch_attn_onex_bwd(a, batch, (hipStream_t)stream);
}
