// The per-row body of the LayerNorm backward, shared by ln_bwd_kernel (norm.hip) and by the side role of the weight-gradient launch
// (gemm.hip, gemm_wgrad_side_kernel): one wave per row, the whole row in registers, width <= 64 * 4 * NC.
//   dx = dres + rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dy * gamma;  dgamma += dy * xhat;  dbeta += dy
// Both callers run THIS text on a row, so dx and its bf16 copy have the same bits whichever launch produced them.
#pragma once
#include "common.h"

// the row operands are read exactly once per launch: nt policy (-DUNIIR_LN_NT=1 for the A/B build)
#ifndef UNIIR_LN_NT
#define UNIIR_LN_NT 0
#endif
#if UNIIR_LN_NT
#define LN_LD(p) __builtin_nontemporal_load(p)
#else
#define LN_LD(p) (*(p))
#endif

struct LnBwdArgs {
    const float* x; long x_stride;
    const float* gamma;
    const void* dy;                 // [rows][width], bf16 or fp32 (DY_F32)
    const float* dres;              // optional, rows at dx_stride
    float* dx; long dx_stride;
    unsigned short* dx_bf16;        // optional [rows][width]
    const float* bscale;            // optional [rows]: the row's factor on what leaves towards the next residual branch
    int rows, width;
    float eps;
    int rms;
    int colsum;                     // the column sums of (bscale *) dx are wanted
};

// one row: loads, the three wave reductions, dx, its bf16 copy, and this wave's column partials (ag: dgamma, ab: dbeta, ac: dx itself)
template <int NC, bool DY_F32, bool EXACT>
DEVINL void ln_bwd_row(const float* __restrict__ x, long x_stride, const float* __restrict__ gamma, const void* __restrict__ dy_,
                       const float* __restrict__ dres, float* __restrict__ dx, long dx_stride, unsigned short* __restrict__ dx_bf16,
                       const void* dx_colsum, int width, float eps, int rms, const float* __restrict__ bscale, long row, int lane,
                       int nchunk, float inv_w, f32x4_t (&ag)[NC], f32x4_t (&ab)[NC], f32x4_t (&ac)[NC]) {
    const float* xr = x + row * x_stride;
    f32x4_t v[NC], d[NC], rs[NC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (EXACT || c < nchunk) {
            v[i] = LN_LD(reinterpret_cast<const f32x4_t*>(xr + 4 * c));
            if (dres) rs[i] = LN_LD(reinterpret_cast<const f32x4_t*>(dres + row * dx_stride + 4 * c));
            s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
            if (DY_F32) {
                d[i] = LN_LD(reinterpret_cast<const f32x4_t*>((const float*)dy_ + row * width + 4 * c));
            } else {
                const u32x2_t pk =
                    LN_LD(reinterpret_cast<const u32x2_t*>((const unsigned short*)dy_ + row * width + 4 * c));
                d[i] = f32x4_t{__uint_as_float(pk[0] << 16), __uint_as_float(pk[0] & 0xffff0000u),
                               __uint_as_float(pk[1] << 16), __uint_as_float(pk[1] & 0xffff0000u)};
            }
        }
    }
    const float mean = rms ? 0.f : wave_sum(s) * inv_w;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (EXACT || c < nchunk) {
            v[i] = v[i] - mean;
            q += (v[i][0] * v[i][0] + v[i][1] * v[i][1]) + (v[i][2] * v[i][2] + v[i][3] * v[i][3]);
        }
    }
    const float rstd = rsqrtf(wave_sum(q) * inv_w + eps);
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (EXACT || c < nchunk) {
            v[i] = v[i] * rstd;  // xhat
            const f32x4_t g = d[i] * *reinterpret_cast<const f32x4_t*>(gamma + 4 * c);
            ag[i] += d[i] * v[i];
            ab[i] += d[i];
            d[i] = g;
            s1 += (g[0] + g[1]) + (g[2] + g[3]);
            s2 += (g[0] * v[i][0] + g[1] * v[i][1]) + (g[2] * v[i][2] + g[3] * v[i][3]);
        }
    }
    const float c1 = rms ? 0.f : wave_sum(s1) * inv_w, c2 = wave_sum(s2) * inv_w;
    // bscale: the row's DropPath factor of the residual BRANCH this gradient enters next (its last linear layer's bias
    // gradient and 16-bit operand see bscale * dx; the fp32 residual gradient itself stays unscaled)
    const float bs = bscale ? bscale[row] : 1.0f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (EXACT || c < nchunk) {
            f32x4_t o = (d[i] - c1 - v[i] * c2) * rstd;
            if (dres) o += rs[i];
            *reinterpret_cast<f32x4_t*>(dx + row * dx_stride + 4 * c) = o;
            if (bscale) o = o * bs;
            if (dx_colsum) ac[i] += o;
            if (dx_bf16) {
                u32x2_t pk = {pack_bf16x2(o[0], o[1]), pack_bf16x2(o[2], o[3])};
                *reinterpret_cast<u32x2_t*>(dx_bf16 + row * width + 4 * c) = pk;
            }
        }
    }
}

// The workgroup's column partials of dgamma, dbeta and (optional) of dx: the NW waves' registers through LDS (red: NW x width
// floats), added in one fixed order, then stored as partial `block` of the [block][pass][width] layout that reduce_partials adds
// up (common.h) -- or, without that scratch, one atomic per column
template <int NC, bool EXACT, int NW>
DEVINL void ln_bwd_col_partials(const LnBwdArgs& a, float* red, int lane, int w, int block, float* part, float* dgamma, float* dbeta,
                                float* dx_colsum, const f32x4_t (&ag)[NC], const f32x4_t (&ab)[NC], const f32x4_t (&ac)[NC]) {
    static_assert(NW == 4 || NW == 8, "four or eight waves per workgroup");
    const int nchunk = a.width >> 2, width = a.width;
    float* mine = red + w * width;
    for (int pass = 0; pass < (a.colsum ? 3 : 2); ++pass) {
        if (pass == 1 && a.rms) continue;      // no beta
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = lane + 64 * i;
            if (EXACT || c < nchunk) *reinterpret_cast<f32x4_t*>(mine + 4 * c) = pass == 0 ? ag[i] : (pass == 1 ? ab[i] : ac[i]);
        }
        __syncthreads();
        float* dst = pass == 0 ? dgamma : (pass == 1 ? dbeta : dx_colsum);
        for (int col = threadIdx.x; col < width; col += 64 * NW) {
            float t = (red[col] + red[width + col]) + (red[2 * width + col] + red[3 * width + col]);
            if (NW == 8) t += (red[4 * width + col] + red[5 * width + col]) + (red[6 * width + col] + red[7 * width + col]);
            // part: this workgroup's three column partials [block][pass][width]; a fixed-order reduction follows (common.h)
            if (part) part[((long)block * 3 + pass) * width + col] = t;
            else unsafeAtomicAdd(dst + col, t);
        }
        __syncthreads();
    }
}

// The side role: workgroup `sb` of `nsb` side workgroups, NW = 8 waves, row r belongs to wave (r mod 8 nsb) -- a fixed assignment,
// so the column partials (and with them dgamma / dbeta / the column sums) are the same bits in every run.
template <int NC>
DEVINL void ln_bwd_side_rows(const LnBwdArgs& a, int sb, int nsb, float* red, float* part, float* dgamma, float* dbeta,
                             float* dx_colsum) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int nchunk = a.width >> 2;
    const float inv_w = 1.0f / (float)a.width;
    f32x4_t ag[NC], ab[NC], ac[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        ag[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        ab[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        ac[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    for (long row = 8L * sb + w; row < a.rows; row += 8L * nsb)
        ln_bwd_row<NC, false, true>(a.x, a.x_stride, a.gamma, a.dy, a.dres, a.dx, a.dx_stride, a.dx_bf16, dx_colsum, a.width, a.eps, a.rms,
                                    a.bscale, row, lane, nchunk, inv_w, ag, ab, ac);
    ln_bwd_col_partials<NC, true, 8>(a, red, lane, w, sb, part, dgamma, dbeta, dx_colsum, ag, ab, ac);
}
