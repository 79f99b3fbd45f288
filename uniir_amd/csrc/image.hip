// Device-side image transform of the encoders' input pipeline: what upstream
// clip._transform (reached from clip_sf.py:25-26, applied per item in src/data/mbeir_dataset.py:92-100) and BLIP's eval
// transform (backbone/transform/blip_transform.py:41-48) do on CPU workers with Pillow + torchvision:
//   Image.resize((ow, oh), BICUBIC) -> centre crop n x n -> x / 255 -> (v - mean) / std -> fp32 [3][n][n]
// on a decoded RGB uint8 image that already sits in HBM.  Integer stage bit-exact with Pillow's 8-bit resample
// (22-bit fixed-point weights, horizontal pass into a uint8 intermediate, then vertical), float stage the same two IEEE
// divisions.  HBM-bound byte work: three small launches per image, only the rows / columns the crop keeps are computed.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>
#include "common.h"
#include "../../include/uniir_hip.h"

#define IMG_BITS 22

DEVINL double keys_cubic(double x) {     // Keys cubic, a = -0.5 (Pillow's BICUBIC)
    const double a = -0.5;
    x = x < 0 ? -x : x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}
static inline int img_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / out_size;
    return (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}
// window bounds + fixed-point weights of output coordinate o of one axis (double arithmetic, no contraction in this translation
// unit, so the table equals the CPU one bit for bit); shared by the per-image and the batched table kernels
DEVINL void img_coeff_row(int in_size, int out_size, int o, int ksize, int* __restrict__ bound2, int* __restrict__ k) {
    const double scale = (double)in_size / out_size;
    const double fscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fscale;
    const double center = (o + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    const int n = xmax - xmin;
    const double inv = 1.0 / fscale;
    double ww = 0.0;
    for (int i = 0; i < n; ++i) ww += keys_cubic((i + xmin - center + 0.5) * inv);
    for (int i = 0; i < ksize; ++i) {
        double v = 0.0;
        if (i < n) {
            v = keys_cubic((i + xmin - center + 0.5) * inv);
            if (ww != 0.0) v = v / ww;
        }
        k[i] = v < 0 ? (int)(-0.5 + v * (1 << IMG_BITS)) : (int)(0.5 + v * (1 << IMG_BITS));
    }
    bound2[0] = xmin;
    bound2[1] = n;
}
// one thread per kept output coordinate o = first + t of one axis
__global__ void img_coeffs_kernel(int in_size, int out_size, int first, int count, int ksize, int* __restrict__ bounds,
                                  int* __restrict__ kk) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count) return;
    img_coeff_row(in_size, out_size, first + t, ksize, bounds + 2 * t, kk + (long)t * ksize);
}
DEVINL unsigned char img_clip8(int acc) {
    const int v = acc >> IMG_BITS;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
// horizontal pass for the kept columns: tmp[y][t][c], y over all source rows the vertical windows touch
__global__ void img_horizontal_kernel(const unsigned char* __restrict__ src, int w, int y0, int rows, int n, int ksize,
                                      const int* __restrict__ bounds, const int* __restrict__ kk,
                                      unsigned char* __restrict__ tmp) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows * n) return;
    const int t = (int)(idx % n), y = (int)(idx / n);
    const int xmin = bounds[2 * t], cnt = bounds[2 * t + 1];
    const int* k = kk + (long)t * ksize;
    const unsigned char* row = src + ((long)(y0 + y) * w + xmin) * 3;
    int a0 = 1 << (IMG_BITS - 1), a1 = a0, a2 = a0;
    for (int i = 0; i < cnt; ++i) {
        const int kv = k[i];
        a0 += row[3 * i] * kv;
        a1 += row[3 * i + 1] * kv;
        a2 += row[3 * i + 2] * kv;
    }
    unsigned char* o = tmp + ((long)y * n + t) * 3;
    o[0] = img_clip8(a0); o[1] = img_clip8(a1); o[2] = img_clip8(a2);
}
// vertical pass + ToTensor + Normalize: out[c][ty][tx] fp32.  tmp rows are relative to y0; `direct` = no vertical resize
__global__ void img_vertical_kernel(const unsigned char* __restrict__ tmp, int y0, int n, int ksize,
                                    const int* __restrict__ bounds, const int* __restrict__ kk, int direct, int top,
                                    float m0, float m1, float m2, float s0, float s1, float s2, float* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * n) return;
    const int tx = idx % n, ty = idx / n;
    unsigned char p0, p1, p2;
    if (direct) {
        const unsigned char* px = tmp + ((long)(top + ty - y0) * n + tx) * 3;
        p0 = px[0]; p1 = px[1]; p2 = px[2];
    } else {
        const int ymin = bounds[2 * ty], cnt = bounds[2 * ty + 1];
        const int* k = kk + (long)ty * ksize;
        int a0 = 1 << (IMG_BITS - 1), a1 = a0, a2 = a0;
        for (int i = 0; i < cnt; ++i) {
            const unsigned char* px = tmp + ((long)(ymin + i - y0) * n + tx) * 3;
            const int kv = k[i];
            a0 += px[0] * kv;
            a1 += px[1] * kv;
            a2 += px[2] * kv;
        }
        p0 = img_clip8(a0); p1 = img_clip8(a1); p2 = img_clip8(a2);
    }
    const long plane = (long)n * n;
    out[idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p0, 255.0f), m0), s0);
    out[plane + idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p1, 255.0f), m1), s1);
    out[2 * plane + idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p2, 255.0f), m2), s2);
}
// same pixel gather when the horizontal size is unchanged: tmp[y][t][c] = src[y0 + y][left + t][c]
__global__ void img_copy_cols_kernel(const unsigned char* __restrict__ src, int w, int y0, int rows, int left, int n,
                                     unsigned char* __restrict__ tmp) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)rows * n * 3) return;
    const int c = (int)(idx % 3);
    const long p = idx / 3;
    const int t = (int)(p % n), y = (int)(p / n);
    tmp[idx] = src[((long)(y0 + y) * w + left + t) * 3 + c];
}

static inline int64_t img_align(int64_t x) { return (x + 255) & ~(int64_t)255; }

extern "C" int64_t uniir_image_workspace_bytes(int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t n) {
    if (h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || n <= 0) return 0;
    const int kx = img_ksize(w, ow), ky = img_ksize(h, oh);
    return img_align(8L * n) * 2 + img_align(4L * n * kx) + img_align(4L * n * ky) + img_align(3L * h * n);
}

extern "C" int uniir_image_preprocess(const void* rgb_u8, int32_t h, int32_t w, int32_t oh, int32_t ow, int32_t top,
                                      int32_t left, int32_t n, const float* mean3, const float* std3, float* out,
                                      void* workspace, int64_t workspace_bytes, void* stream) {
    if (!rgb_u8 || !mean3 || !std3 || !out || !workspace) return UNIIR_EINVAL;
    if (h <= 0 || w <= 0 || oh <= 0 || ow <= 0 || n <= 0) return UNIIR_EINVAL;
    if (top < 0 || left < 0 || top + n > oh || left + n > ow) return UNIIR_ESHAPE;
    if (workspace_bytes < uniir_image_workspace_bytes(h, w, oh, ow, n) || ((uintptr_t)workspace & 15)) return UNIIR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int kx = img_ksize(w, ow), ky = img_ksize(h, oh);
    char* ws = (char*)workspace;
    int* bx = (int*)ws;                 ws += img_align(8L * n);
    int* by = (int*)ws;                 ws += img_align(8L * n);
    int* cx = (int*)ws;                 ws += img_align(4L * n * kx);
    int* cy = (int*)ws;                 ws += img_align(4L * n * ky);
    unsigned char* tmp = (unsigned char*)ws;
    const bool hres = ow != w, vres = oh != h;
    // source rows the vertical windows of the kept output rows can touch (host copy of the bound arithmetic)
    int y0 = top, y1 = top + n;
    if (vres) {
        const double scale = (double)h / oh, fscale = scale < 1.0 ? 1.0 : scale, support = 2.0 * fscale;
        y0 = (int)((top + 0.5) * scale - support + 0.5);
        if (y0 < 0) y0 = 0;
        y1 = (int)((top + n - 1 + 0.5) * scale + support + 0.5);
        if (y1 > h) y1 = h;
    }
    const int rows = y1 - y0;
    if (hres) hipLaunchKernelGGL(img_coeffs_kernel, dim3((n + 63) / 64), dim3(64), 0, st, w, ow, left, n, kx, bx, cx);
    if (vres) hipLaunchKernelGGL(img_coeffs_kernel, dim3((n + 63) / 64), dim3(64), 0, st, h, oh, top, n, ky, by, cy);
    if (hres)
        hipLaunchKernelGGL(img_horizontal_kernel, dim3((unsigned)(((long)rows * n + 255) / 256)), dim3(256), 0, st,
                           (const unsigned char*)rgb_u8, w, y0, rows, n, kx, bx, cx, tmp);
    else
        hipLaunchKernelGGL(img_copy_cols_kernel, dim3((unsigned)(((long)rows * n * 3 + 255) / 256)), dim3(256), 0, st,
                           (const unsigned char*)rgb_u8, w, y0, rows, left, n, tmp);
    hipLaunchKernelGGL(img_vertical_kernel, dim3((n * n + 255) / 256), dim3(256), 0, st, tmp, y0, n, ky, by, cy,
                       vres ? 0 : 1, top, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out);
    HIP_LAUNCH_CHECK();
    return UNIIR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Batched form (include/uniir_hip.h [IMAGE]): one descriptor per image (source box, resized size, window, flip, output slot), one
// plan per image (table / intermediate offsets in the workspace, touched source rows and columns), three launches per batch
// whatever its size.  Semantics of Pillow's crop(box).resize(): every window is clamped at the BOX edges, so all coordinates
// below are relative to the box and only the pixel fetch adds (box_top, box_left).
// ------------------------------------------------------------------------------------------------------------------------------
#define IMGB_ROWS 32              // box rows per workgroup of the horizontal pass
#define IMGB_MAX_COLS 16384       // widest row segment the horizontal pass stages (pixels)
#define IMGB_STAGE_BYTES 49408    // >= IMGB_MAX_COLS * 3 + 15 rounded up to 16: one row always fits
#define IMGB_MAX_N 2048
#define IMGB_MAX_SIDE (1 << 20)

// all coefficient tables of the batch: grid (image, axis, 64 kept coordinates)
__global__ __launch_bounds__(64) void img_batch_coeffs_kernel(const uniir_image_desc* __restrict__ descs,
                                                              const uniir_image_plan* __restrict__ plans, int n,
                                                              unsigned char* __restrict__ ws) {
    const int t = blockIdx.z * 64 + threadIdx.x;
    if (t >= n) return;
    const uniir_image_desc d = descs[blockIdx.x];
    const uniir_image_plan pl = plans[blockIdx.x];
    if (blockIdx.y == 0) {
        if (pl.kx == 0) return;
        img_coeff_row(d.box_w, d.ow, d.left + t, pl.kx, (int*)(ws + pl.bx_off) + 2 * t, (int*)(ws + pl.cx_off) + (long)t * pl.kx);
    } else {
        if (pl.ky == 0) return;
        img_coeff_row(d.box_h, d.oh, d.top + t, pl.ky, (int*)(ws + pl.by_off) + 2 * t, (int*)(ws + pl.cy_off) + (long)t * pl.ky);
    }
}
// all horizontal passes: grid (image, chunk of IMGB_ROWS touched box rows).  The row segments [x0, x0 + cols) are staged in LDS with
// 16-byte loads (whole aligned chunks; the ragged first / last chunk byte-wise, nothing outside the segment is read), several
// rows per stage, and every kept column takes its taps from there.  tmp[y][t][c], y relative to plan.y0; without a horizontal
// resize the kept columns are copied.
__global__ __launch_bounds__(256) void img_batch_horizontal_kernel(const unsigned char* __restrict__ packed,
                                                                   const uniir_image_desc* __restrict__ descs,
                                                                   const uniir_image_plan* __restrict__ plans, int n,
                                                                   unsigned char* __restrict__ ws) {
    __shared__ __attribute__((aligned(16))) unsigned char stage[IMGB_STAGE_BYTES];
    const uniir_image_plan pl = plans[blockIdx.x];
    const int r0 = blockIdx.y * IMGB_ROWS;
    if (r0 >= pl.rows) return;                      // an image with fewer touched rows than the largest of the batch
    const uniir_image_desc d = descs[blockIdx.x];
    const int r1 = r0 + IMGB_ROWS < pl.rows ? r0 + IMGB_ROWS : pl.rows;
    const int seg = pl.cols * 3;                    // bytes of one row segment
    const int stride = (seg + 30) & ~15;            // + up to 15 bytes of misalignment, rounded up to 16
    const int chunks = stride >> 4;
    const int per_stage = IMGB_STAGE_BYTES / stride;
    const unsigned char* src = packed + d.offset;   // 16-byte aligned
    const int* bx = (const int*)(ws + pl.bx_off);
    const int* cx = (const int*)(ws + pl.cx_off);
    unsigned char* tmp = ws + pl.tmp_off;
    for (int s0 = r0; s0 < r1; s0 += per_stage) {
        const int ns = per_stage < r1 - s0 ? per_stage : r1 - s0;
        const long first = ((long)(d.box_top + pl.y0 + s0) * d.w + d.box_left + pl.x0) * 3;     // segment start of row s0
        for (int idx = threadIdx.x; idx < ns * chunks; idx += 256) {
            const int r = idx / chunks, c = idx - r * chunks;
            const long b0 = first + (long)r * d.w * 3;
            const long a = (b0 & ~15L) + 16L * c;
            unsigned char* dst = stage + r * stride + 16 * c;
            if (a >= b0 && a + 16 <= b0 + seg) {
                *(uint4*)dst = *(const uint4*)(src + a);
            } else {
                for (int b = 0; b < 16; ++b)
                    if (a + b >= b0 && a + b < b0 + seg) dst[b] = src[a + b];
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < ns * n; idx += 256) {
            const int r = idx / n, t = idx - r * n;
            const long b0 = first + (long)r * d.w * 3;
            const unsigned char* row = stage + r * stride + (int)(b0 & 15);      // box column x0
            unsigned char* o = tmp + ((long)(s0 + r) * n + t) * 3;
            if (pl.kx) {
                const int xmin = bx[2 * t], cnt = bx[2 * t + 1];
                const int* k = cx + (long)t * pl.kx;
                const unsigned char* px = row + (xmin - pl.x0) * 3;
                int a0 = 1 << (IMG_BITS - 1), a1 = a0, a2 = a0;
                for (int i = 0; i < cnt; ++i) {
                    const int kv = k[i];
                    a0 += px[3 * i] * kv;
                    a1 += px[3 * i + 1] * kv;
                    a2 += px[3 * i + 2] * kv;
                }
                o[0] = img_clip8(a0); o[1] = img_clip8(a1); o[2] = img_clip8(a2);
            } else {
                const unsigned char* px = row + t * 3;      // x0 == left
                o[0] = px[0]; o[1] = px[1]; o[2] = px[2];
            }
        }
        __syncthreads();
    }
}
// all vertical passes + ToTensor + Normalize: grid (image, 256 output pixels), x fastest, so the fp32 stores are coalesced; the
// flip mirrors the column that is READ
// U8: the same pixels as bytes, u8out[image][ty][tx][3] by position in the table (the augmentation ops run on them before ToTensor)
template <bool U8>
__global__ __launch_bounds__(256) void img_batch_vertical_kernel(const uniir_image_desc* __restrict__ descs,
                                                                 const uniir_image_plan* __restrict__ plans, int n,
                                                                 const unsigned char* __restrict__ ws, float m0, float m1, float m2,
                                                                 float s0, float s1, float s2, float* __restrict__ out,
                                                                 unsigned char* __restrict__ u8out) {
    const int idx = blockIdx.y * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const uniir_image_desc d = descs[blockIdx.x];
    const uniir_image_plan pl = plans[blockIdx.x];
    const int ty = idx / n, tx = idx - ty * n;
    const int sx = d.flip ? n - 1 - tx : tx;
    const unsigned char* tmp = ws + pl.tmp_off;
    unsigned char p0, p1, p2;
    if (pl.ky == 0) {
        const unsigned char* px = tmp + ((long)(d.top + ty - pl.y0) * n + sx) * 3;
        p0 = px[0]; p1 = px[1]; p2 = px[2];
    } else {
        const int* by = (const int*)(ws + pl.by_off);
        const int ymin = by[2 * ty], cnt = by[2 * ty + 1];
        const int* k = (const int*)(ws + pl.cy_off) + (long)ty * pl.ky;
        int a0 = 1 << (IMG_BITS - 1), a1 = a0, a2 = a0;
        for (int i = 0; i < cnt; ++i) {
            const unsigned char* px = tmp + ((long)(ymin + i - pl.y0) * n + sx) * 3;
            const int kv = k[i];
            a0 += px[0] * kv;
            a1 += px[1] * kv;
            a2 += px[2] * kv;
        }
        p0 = img_clip8(a0); p1 = img_clip8(a1); p2 = img_clip8(a2);
    }
    const long plane = (long)n * n;
    if (U8) {
        unsigned char* b = u8out + ((long)blockIdx.x * plane + idx) * 3;
        b[0] = p0; b[1] = p1; b[2] = p2;
        return;
    }
    float* o = out + (long)d.out_index * 3 * plane;
    o[idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p0, 255.0f), m0), s0);
    o[plane + idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p1, 255.0f), m1), s1);
    o[2 * plane + idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p2, 255.0f), m2), s2);
}

// source coordinates [lo, lo + cnt) that the windows of the kept outputs [first, first + n) of one axis touch, and the window
// capacity (host copy of the bound arithmetic of img_coeff_row); an axis that keeps its size is read directly: ksize 0
static inline void img_axis_range(int in_size, int out_size, int first, int n, int* lo, int* cnt, int* ksize) {
    if (in_size == out_size) {
        *lo = first; *cnt = n; *ksize = 0;
        return;
    }
    const double scale = (double)in_size / out_size, fscale = scale < 1.0 ? 1.0 : scale, support = 2.0 * fscale;
    int a = (int)((first + 0.5) * scale - support + 0.5);
    if (a < 0) a = 0;
    int b = (int)((first + n - 1 + 0.5) * scale + support + 0.5);
    if (b > in_size) b = in_size;
    *lo = a; *cnt = b - a; *ksize = img_ksize(in_size, out_size);
}

extern "C" int uniir_image_batch_plan(const uniir_image_desc* descs, int32_t count, int32_t n, int32_t out_items,
                                      int64_t packed_bytes, uniir_image_plan* plans, uniir_image_batch_info* info) {
    if (!info || count < 0 || n <= 0 || out_items <= 0 || packed_bytes < 0) return UNIIR_EINVAL;
    if (count > 0 && (!descs || !plans)) return UNIIR_EINVAL;
    if (n > IMGB_MAX_N) return UNIIR_EUNSUPPORTED;
    int64_t ws = 0;
    int max_rows = 0;
    std::vector<int32_t> slots((size_t)count);
    for (int i = 0; i < count; ++i) {
        const uniir_image_desc& d = descs[i];
        if (d.h <= 0 || d.w <= 0 || d.box_w <= 0 || d.box_h <= 0 || d.oh <= 0 || d.ow <= 0) return UNIIR_EINVAL;
        if ((d.flip != 0 && d.flip != 1) || d.offset < 0 || (d.offset & 15)) return UNIIR_EINVAL;
        if (d.out_index < 0 || d.out_index >= out_items) return UNIIR_EINVAL;
        if (d.h > IMGB_MAX_SIDE || d.w > IMGB_MAX_SIDE || d.oh > IMGB_MAX_SIDE || d.ow > IMGB_MAX_SIDE) return UNIIR_EUNSUPPORTED;
        if (d.box_left < 0 || d.box_top < 0 || (int64_t)d.box_left + d.box_w > d.w || (int64_t)d.box_top + d.box_h > d.h)
            return UNIIR_ESHAPE;
        if (d.top < 0 || d.left < 0 || (int64_t)d.top + n > d.oh || (int64_t)d.left + n > d.ow) return UNIIR_ESHAPE;
        if (d.offset + 3 * (int64_t)d.h * d.w > packed_bytes) return UNIIR_ESHAPE;
        slots[i] = d.out_index;
    }
    std::sort(slots.begin(), slots.end());
    for (int i = 1; i < count; ++i)
        if (slots[i] == slots[i - 1]) return UNIIR_EINVAL;
    for (int i = 0; i < count; ++i) {
        const uniir_image_desc& d = descs[i];
        uniir_image_plan& p = plans[i];
        img_axis_range(d.box_w, d.ow, d.left, n, &p.x0, &p.cols, &p.kx);
        img_axis_range(d.box_h, d.oh, d.top, n, &p.y0, &p.rows, &p.ky);
        if (p.cols > IMGB_MAX_COLS) return UNIIR_EUNSUPPORTED;
        p.bx_off = ws; ws += img_align(8L * n);
        p.by_off = ws; ws += img_align(8L * n);
        p.cx_off = ws; ws += img_align(4L * n * p.kx);
        p.cy_off = ws; ws += img_align(4L * n * p.ky);
        p.tmp_off = ws; ws += img_align(3L * p.rows * n);
        if (p.rows > max_rows) max_rows = p.rows;
    }
    info->workspace_bytes = ws;
    info->count = count; info->n = n; info->out_items = out_items;
    info->max_rows = max_rows;
    info->launches = count > 0 ? 3 : 0;
    info->reserved = 0;
    return UNIIR_OK;
}

extern "C" int uniir_image_preprocess_batch(const void* packed_u8, const uniir_image_desc* descs, const uniir_image_plan* plans,
                                            const uniir_image_batch_info* info, const float* mean3, const float* std3, float* out,
                                            void* workspace, int64_t workspace_bytes, void* stream) {
    if (!info || info->count < 0) return UNIIR_EINVAL;
    if (info->count == 0) return UNIIR_OK;
    if (!packed_u8 || !descs || !plans || !mean3 || !std3 || !out || !workspace) return UNIIR_EINVAL;
    if (info->n <= 0 || info->n > IMGB_MAX_N || info->out_items <= 0 || info->max_rows <= 0) return UNIIR_EINVAL;
    if (((uintptr_t)packed_u8 & 15) || ((uintptr_t)workspace & 255) || workspace_bytes < info->workspace_bytes) return UNIIR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int n = info->n;
    const unsigned count = (unsigned)info->count;
    unsigned char* ws = (unsigned char*)workspace;
    hipLaunchKernelGGL(img_batch_coeffs_kernel, dim3(count, 2, (n + 63) / 64), dim3(64), 0, st, descs, plans, n, ws);
    hipLaunchKernelGGL(img_batch_horizontal_kernel, dim3(count, (info->max_rows + IMGB_ROWS - 1) / IMGB_ROWS), dim3(256), 0, st,
                       (const unsigned char*)packed_u8, descs, plans, n, ws);
    hipLaunchKernelGGL(img_batch_vertical_kernel<false>, dim3(count, (n * n + 255) / 256), dim3(256), 0, st, descs, plans, n,
                       (const unsigned char*)ws, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out, (unsigned char*)nullptr);
    HIP_LAUNCH_CHECK();
    return UNIIR_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// Train-time augmentation (include/uniir_hip.h [IMAGE]): one uniir_image_aug record per image, up to four op
// slots applied in order on uint8 [count][n][n][3].  Per slot two launches whatever the batch: statistics (per-channel histograms
// in LDS -> the 256-entry tables of the ops that need them) and apply (table lookup, fixed-point bilinear gather, 3x3 filter or
// copy, by op code), ping-ponging between two buffers.  Every formula below is restated in numpy by tests/randaugment_ref.py and
// compared byte for byte: fp64 / fp32 products are rounded before they are summed (the __d*_rn / __f*_rn forms say so).
// ------------------------------------------------------------------------------------------------------------------------------
#define AUG_STAT_THREADS 1024
#define AUG_STAT_WAVES (AUG_STAT_THREADS / 64)
#define AUG_FILL 128
#define AUG_MAX_ARG 1e6

DEVINL bool aug_needs_stats(int op) {
    return op == UNIIR_AUG_AUTOCONTRAST || op == UNIIR_AUG_EQUALIZE || op == UNIIR_AUG_AUTOCONTRAST_PIL;
}
// one workgroup per image; images whose op of this slot needs no histogram leave at once.  lut[image][3][256]
__global__ __launch_bounds__(AUG_STAT_THREADS) void img_aug_stats_kernel(const unsigned char* __restrict__ src,
                                                                         const uniir_image_aug* __restrict__ table, int slot, int n,
                                                                         unsigned char* __restrict__ lut) {
    __shared__ unsigned int sub[AUG_STAT_WAVES][3][256];        // one histogram per wave: integer LDS atomics, order-independent
    __shared__ unsigned int hist[3][256];
    __shared__ unsigned int scan[256];
    __shared__ int lohi[2];
    const int op = table[blockIdx.x].slot[slot].op;
    if (!aug_needs_stats(op)) return;
    const int t = threadIdx.x;
    for (int i = t; i < AUG_STAT_WAVES * 3 * 256; i += AUG_STAT_THREADS) (&sub[0][0][0])[i] = 0;
    __syncthreads();
    const long pixels = (long)n * n;
    const unsigned char* img = src + (long)blockIdx.x * pixels * 3;
    unsigned int(*mine)[256] = sub[t >> 6];
    if ((pixels & 3) == 0 && ((uintptr_t)img & 3) == 0) {      // even n, image on a dword boundary: 4 pixels = 3 dwords
        const uint32_t* words = (const uint32_t*)img;
#pragma unroll 2
        for (long g = t; g < pixels / 4; g += AUG_STAT_THREADS) {
            const uint32_t w0 = words[3 * g], w1 = words[3 * g + 1], w2 = words[3 * g + 2];     // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
            atomicAdd(&mine[0][w0 & 255], 1u);
            atomicAdd(&mine[1][(w0 >> 8) & 255], 1u);
            atomicAdd(&mine[2][(w0 >> 16) & 255], 1u);
            atomicAdd(&mine[0][w0 >> 24], 1u);
            atomicAdd(&mine[1][w1 & 255], 1u);
            atomicAdd(&mine[2][(w1 >> 8) & 255], 1u);
            atomicAdd(&mine[0][(w1 >> 16) & 255], 1u);
            atomicAdd(&mine[1][w1 >> 24], 1u);
            atomicAdd(&mine[2][w2 & 255], 1u);
            atomicAdd(&mine[0][(w2 >> 8) & 255], 1u);
            atomicAdd(&mine[1][(w2 >> 16) & 255], 1u);
            atomicAdd(&mine[2][w2 >> 24], 1u);
        }
    } else {
        for (long p = t; p < pixels; p += AUG_STAT_THREADS) {
            atomicAdd(&mine[0][img[3 * p]], 1u);
            atomicAdd(&mine[1][img[3 * p + 1]], 1u);
            atomicAdd(&mine[2][img[3 * p + 2]], 1u);
        }
    }
    __syncthreads();
    for (int i = t; i < 3 * 256; i += AUG_STAT_THREADS) {
        unsigned int s = 0;
        for (int w = 0; w < AUG_STAT_WAVES; ++w) s += (&sub[w][0][0])[i];
        (&hist[0][0])[i] = s;
    }
    __syncthreads();
    for (int c = 0; c < 3; ++c) {
        if (t == 0) { lohi[0] = 256; lohi[1] = -1; }
        if (t < 256) scan[t] = hist[c][t];
        __syncthreads();
        if (t < 256 && hist[c][t]) {
            atomicMin(&lohi[0], t);
            atomicMax(&lohi[1], t);
        }
        for (int off = 1; off < 256; off <<= 1) {               // inclusive prefix sums of the 256 bins
            const unsigned int a = (t < 256 && t >= off) ? scan[t - off] : 0;
            __syncthreads();
            if (t < 256) scan[t] += a;
            __syncthreads();
        }
        if (t < 256) {
            const int lo = lohi[0], hi = lohi[1];
            int v = t;                                          // an unchanged channel: the identity table
            if (op == UNIIR_AUG_EQUALIZE) {
                const unsigned int step = (scan[255] - hist[c][hi]) / 255u;
                if (step) {
                    const unsigned int q = (step / 2 + scan[t] - hist[c][t]) / step;
                    v = q > 255u ? 255 : (int)q;
                }
            } else if (hi > lo) {
                const double scale = __ddiv_rn(255.0, (double)(hi - lo));
                const double off = op == UNIIR_AUG_AUTOCONTRAST_PIL ? __dmul_rn(-(double)lo, scale)
                                                                    : __dmul_rn((double)((256 - lo) % 256), scale);
                double f = __dadd_rn(__dmul_rn((double)t, scale), off);
                f = f < 0.0 ? 0.0 : (f > 255.0 ? 255.0 : f);
                v = (int)f;
            }
            lut[((long)blockIdx.x * 3 + c) * 256 + t] = (unsigned char)v;
        }
        __syncthreads();                                        // scan and lohi are reused by the next channel
    }
}

DEVINL long aug_fix(double v) {                                  // rint (half to even), saturated to int32
    v = rint(v);
    v = v < -2147483648.0 ? -2147483648.0 : (v > 2147483647.0 ? 2147483647.0 : v);
    return (long)v;
}
DEVINL int aug_tap(const unsigned char* __restrict__ img, int n, long yy, long xx, int c) {
    return (yy >= 0 && yy < n && xx >= 0 && xx < n) ? img[(yy * n + xx) * 3 + c] : AUG_FILL;
}
DEVINL int aug_reflect(int i, int n) { return i < 0 ? (n > 1 ? 1 : 0) : (i >= n ? (n > 1 ? n - 2 : 0) : i); }
// grid (image, 256 pixels): dst[image][y][x][:] = op(src[image]) for the op of this slot
__global__ __launch_bounds__(256) void img_aug_apply_kernel(const unsigned char* __restrict__ src,
                                                            const uniir_image_aug* __restrict__ table, int slot, int n,
                                                            const unsigned char* __restrict__ lut, unsigned char* __restrict__ dst) {
    const int idx = blockIdx.y * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const uniir_image_aug_slot s = table[blockIdx.x].slot[slot];
    const long base = (long)blockIdx.x * n * n * 3;
    const unsigned char* img = src + base;
    const unsigned char* px = img + (long)idx * 3;
    unsigned char* o = dst + base + (long)idx * 3;
    const int y = idx / n, x = idx - y * n;
    int r0 = px[0], r1 = px[1], r2 = px[2];
    switch (s.op) {
    case UNIIR_AUG_AUTOCONTRAST:
    case UNIIR_AUG_AUTOCONTRAST_PIL:
    case UNIIR_AUG_EQUALIZE: {
        const unsigned char* l = lut + (long)blockIdx.x * 768;
        r0 = l[r0]; r1 = l[256 + r1]; r2 = l[512 + r2];
        break;
    }
    case UNIIR_AUG_BRIGHTNESS: {
        const float f = (float)s.p[0];
        float v0 = __fmul_rn((float)r0, f), v1 = __fmul_rn((float)r1, f), v2 = __fmul_rn((float)r2, f);
        r0 = (int)(v0 < 0.f ? 0.f : (v0 > 255.f ? 255.f : v0));
        r1 = (int)(v1 < 0.f ? 0.f : (v1 > 255.f ? 255.f : v1));
        r2 = (int)(v2 < 0.f ? 0.f : (v2 > 255.f ? 255.f : v2));
        break;
    }
    case UNIIR_AUG_SHARPNESS: {
        if (s.p[0] == 1.0) break;
        const float k = __fdiv_rn(1.0f, 13.0f), kc = __fdiv_rn(5.0f, 13.0f), f = (float)s.p[0];
        const bool blend = s.p[0] != 0.0;
        if (blend && (x == 0 || y == 0 || x == n - 1 || y == n - 1)) break;     // the border keeps the input
        int in3[3] = {r0, r1, r2}, out3[3];
        for (int c = 0; c < 3; ++c) {
            float acc = 0.f;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const float p = (float)img[((long)aug_reflect(y + dy, n) * n + aug_reflect(x + dx, n)) * 3 + c];
                    acc = __fadd_rn(acc, __fmul_rn(p, (dy == 0 && dx == 0) ? kc : k));
                }
            float d = rintf(acc);
            d = d < 0.f ? 0.f : (d > 255.f ? 255.f : d);
            if (blend) {
                float v = truncf(__fadd_rn(d, __fmul_rn(f, __fsub_rn((float)in3[c], d))));
                v = v < -2147483648.f ? -2147483648.f : (v > 2147483520.f ? 2147483520.f : v);
                out3[c] = (int)((long)v & 255);
            } else {
                out3[c] = (int)d;
            }
        }
        r0 = out3[0]; r1 = out3[1]; r2 = out3[2];
        break;
    }
    case UNIIR_AUG_SHEAR_X:
    case UNIIR_AUG_SHEAR_Y:
    case UNIIR_AUG_TRANSLATE_X:
    case UNIIR_AUG_TRANSLATE_Y:
    case UNIIR_AUG_ROTATE: {
        const double xd = (double)x, yd = (double)y;
        const long X = (aug_fix(__dmul_rn(__dadd_rn(__dmul_rn(s.p[1], yd), s.p[2]), 1024.0)) + 16 +
                        aug_fix(__dmul_rn(__dmul_rn(s.p[0], xd), 1024.0))) >> 5;
        const long Y = (aug_fix(__dmul_rn(__dadd_rn(__dmul_rn(s.p[4], yd), s.p[5]), 1024.0)) + 16 +
                        aug_fix(__dmul_rn(__dmul_rn(s.p[3], xd), 1024.0))) >> 5;
        const long sx = X >> 5, sy = Y >> 5;
        const int fx = (int)(X & 31), fy = (int)(Y & 31);
        // rint(wy * wx * 32768) of the 1/32 fractions: exact integers that sum to 32768, the correction never applies
        const int w00 = (32 - fy) * (32 - fx) * 32, w01 = (32 - fy) * fx * 32, w10 = fy * (32 - fx) * 32, w11 = fy * fx * 32;
        int out3[3];
        for (int c = 0; c < 3; ++c) {
            const int acc = aug_tap(img, n, sy, sx, c) * w00 + aug_tap(img, n, sy, sx + 1, c) * w01 +
                            aug_tap(img, n, sy + 1, sx, c) * w10 + aug_tap(img, n, sy + 1, sx + 1, c) * w11;
            out3[c] = (acc + 16384) >> 15;
        }
        r0 = out3[0]; r1 = out3[1]; r2 = out3[2];
        break;
    }
    default: break;                                             // Identity: a copy
    }
    o[0] = (unsigned char)r0; o[1] = (unsigned char)r1; o[2] = (unsigned char)r2;
}
// ToTensor + Normalize of the augmented bytes: the expression and the x-fastest store order of img_batch_vertical_kernel
__global__ __launch_bounds__(256) void img_aug_normalize_kernel(const unsigned char* __restrict__ src,
                                                                const uniir_image_desc* __restrict__ descs, int n, float m0, float m1,
                                                                float m2, float s0, float s1, float s2, float* __restrict__ out) {
    const int idx = blockIdx.y * 256 + threadIdx.x;
    if (idx >= n * n) return;
    const long plane = (long)n * n;
    const unsigned char* px = src + ((long)blockIdx.x * plane + idx) * 3;
    const unsigned char p0 = px[0], p1 = px[1], p2 = px[2];
    float* o = out + (long)descs[blockIdx.x].out_index * 3 * plane;
    o[idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p0, 255.0f), m0), s0);
    o[plane + idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p1, 255.0f), m1), s1);
    o[2 * plane + idx] = __fdiv_rn(__fsub_rn(__fdiv_rn((float)p2, 255.0f), m2), s2);
}

// forward matrix of a warp op -> its fp64 inverse (every product rounded before it is summed: no contraction in this file)
static void aug_inverse(int op, double arg, int n, double* p) {
    double a00 = 1, a01 = 0, a02 = 0, a10 = 0, a11 = 1, a12 = 0;
    if (op == UNIIR_AUG_SHEAR_X) a01 = (double)(float)arg;
    else if (op == UNIIR_AUG_SHEAR_Y) a10 = (double)(float)arg;
    else if (op == UNIIR_AUG_TRANSLATE_X) a02 = (double)(float)-arg;
    else if (op == UNIIR_AUG_TRANSLATE_Y) a12 = (double)(float)-arg;
    else {
        const double cx = n / 2.0, cy = n / 2.0, rad = arg * (3.141592653589793 / 180.0);
        const double a = cos(rad), b = sin(rad);
        a00 = a; a01 = b; a02 = (1 - a) * cx - b * cy;
        a10 = -b; a11 = a; a12 = b * cx + (1 - a) * cy;
    }
    double d = a00 * a11 - a01 * a10;
    d = d != 0 ? 1.0 / d : 0.0;
    const double i00 = a11 * d, i11 = a00 * d, i01 = a01 * -d, i10 = a10 * -d;
    p[0] = i00; p[1] = i01; p[2] = -i00 * a02 - i01 * a12;
    p[3] = i10; p[4] = i11; p[5] = -i10 * a02 - i11 * a12;
}

extern "C" int uniir_image_aug_plan(const int32_t* ops, const double* args, int32_t count, int32_t slots, int32_t n,
                                    uniir_image_aug* table, uniir_image_aug_info* info) {
    if (!info || count < 0 || n <= 0 || slots < 0 || slots > UNIIR_AUG_MAX_SLOTS) return UNIIR_EINVAL;
    if (count > 0 && (!table || (slots > 0 && (!ops || !args)))) return UNIIR_EINVAL;
    if (n > IMGB_MAX_N) return UNIIR_EUNSUPPORTED;
    for (long i = 0; i < (long)count * slots; ++i) {
        if (ops[i] < 0 || ops[i] >= UNIIR_AUG_OPS || !std::isfinite(args[i])) return UNIIR_EINVAL;
    }
    for (long i = 0; i < (long)count * slots; ++i)
        if (fabs(args[i]) > AUG_MAX_ARG) return UNIIR_EUNSUPPORTED;
    for (int i = 0; i < count; ++i) {
        uniir_image_aug& rec = table[i];
        memset(&rec, 0, sizeof(rec));                           // unused slots: Identity
        for (int k = 0; k < slots; ++k) {
            const int op = ops[(long)i * slots + k];
            const double arg = args[(long)i * slots + k];
            rec.slot[k].op = op;
            if (op == UNIIR_AUG_BRIGHTNESS || op == UNIIR_AUG_SHARPNESS) rec.slot[k].p[0] = arg;
            else if (op >= UNIIR_AUG_SHEAR_X && op <= UNIIR_AUG_ROTATE) aug_inverse(op, arg, n, rec.slot[k].p);
        }
    }
    info->workspace_bytes = count > 0 ? 2 * img_align(3L * count * n * n) + img_align(768L * count) : 0;
    info->count = count; info->n = n; info->slots = slots;
    info->launches = count > 0 ? 2 * slots : 0;
    info->launches_preprocess = count > 0 ? 3 + 2 * slots + 1 : 0;
    info->reserved = 0;
    return UNIIR_OK;
}

// slot k reads what slot k - 1 wrote (`first` for k = 0, never written) and writes `even` / `odd` by its parity -> the buffer the
// last slot wrote
static const unsigned char* aug_run_slots(hipStream_t st, const unsigned char* first, unsigned char* even, unsigned char* odd,
                                          const uniir_image_aug* table, unsigned char* lut, int count, int n, int slots) {
    const dim3 grid((unsigned)count, (unsigned)((n * n + 255) / 256));
    const unsigned char* cur = first;
    for (int k = 0; k < slots; ++k) {
        unsigned char* nxt = (k & 1) ? odd : even;
        hipLaunchKernelGGL(img_aug_stats_kernel, dim3((unsigned)count), dim3(AUG_STAT_THREADS), 0, st, cur, table, k, n, lut);
        hipLaunchKernelGGL(img_aug_apply_kernel, grid, dim3(256), 0, st, cur, table, k, n, (const unsigned char*)lut, nxt);
        cur = nxt;
    }
    return cur;
}

extern "C" int uniir_image_augment_batch(const void* in_u8, const uniir_image_aug* table, const uniir_image_aug_info* info,
                                         void* out_u8, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!info || info->count < 0) return UNIIR_EINVAL;
    if (info->count == 0) return UNIIR_OK;
    if (!in_u8 || !table || !out_u8 || !workspace || in_u8 == out_u8) return UNIIR_EINVAL;
    if (info->n <= 0 || info->n > IMGB_MAX_N || info->slots < 0 || info->slots > UNIIR_AUG_MAX_SLOTS) return UNIIR_EINVAL;
    if (((uintptr_t)workspace & 255) || workspace_bytes < info->workspace_bytes) return UNIIR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int n = info->n, count = info->count;
    const int64_t buf = img_align(3L * count * n * n);
    unsigned char* ws = (unsigned char*)workspace;
    if (info->slots == 0) {
        if (hipMemcpyAsync(out_u8, in_u8, 3L * count * n * n, hipMemcpyDeviceToDevice, st) != hipSuccess) return UNIIR_ELAUNCH;
        return UNIIR_OK;
    }
    unsigned char* o = (unsigned char*)out_u8;                  // the last slot writes out_u8: it is `even` for an odd slot count
    aug_run_slots(st, (const unsigned char*)in_u8, (info->slots & 1) ? o : ws, (info->slots & 1) ? ws : o, table, ws + 2 * buf, count,
                  n, info->slots);
    HIP_LAUNCH_CHECK();
    return UNIIR_OK;
}

extern "C" int uniir_image_preprocess_batch_aug(const void* packed_u8, const uniir_image_desc* descs, const uniir_image_plan* plans,
                                                const uniir_image_batch_info* info, const uniir_image_aug* aug,
                                                const uniir_image_aug_info* aug_info, const float* mean3, const float* std3,
                                                float* out, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!info || !aug_info || info->count < 0 || aug_info->count != info->count) return UNIIR_EINVAL;
    if (info->count == 0) return UNIIR_OK;
    if (!packed_u8 || !descs || !plans || !aug || !mean3 || !std3 || !out || !workspace) return UNIIR_EINVAL;
    if (info->n <= 0 || info->n > IMGB_MAX_N || info->out_items <= 0 || info->max_rows <= 0 || aug_info->n != info->n)
        return UNIIR_EINVAL;
    if (aug_info->slots < 0 || aug_info->slots > UNIIR_AUG_MAX_SLOTS) return UNIIR_EINVAL;
    if (((uintptr_t)packed_u8 & 15) || ((uintptr_t)workspace & 255) ||
        workspace_bytes < info->workspace_bytes + aug_info->workspace_bytes)
        return UNIIR_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int n = info->n;
    const unsigned count = (unsigned)info->count;
    unsigned char* ws = (unsigned char*)workspace;
    const int64_t buf = img_align(3L * count * n * n);
    unsigned char* u0 = ws + info->workspace_bytes;              // info->workspace_bytes is a multiple of 256
    unsigned char* u1 = u0 + buf;
    unsigned char* lut = u1 + buf;
    const dim3 grid(count, (n * n + 255) / 256);
    hipLaunchKernelGGL(img_batch_coeffs_kernel, dim3(count, 2, (n + 63) / 64), dim3(64), 0, st, descs, plans, n, ws);
    hipLaunchKernelGGL(img_batch_horizontal_kernel, dim3(count, (info->max_rows + IMGB_ROWS - 1) / IMGB_ROWS), dim3(256), 0, st,
                       (const unsigned char*)packed_u8, descs, plans, n, ws);
    hipLaunchKernelGGL(img_batch_vertical_kernel<true>, grid, dim3(256), 0, st, descs, plans, n, (const unsigned char*)ws, 0.f, 0.f,
                       0.f, 1.f, 1.f, 1.f, (float*)nullptr, u0);
    const unsigned char* fin = aug_run_slots(st, u0, u1, u0, aug, lut, (int)count, n, aug_info->slots);
    hipLaunchKernelGGL(img_aug_normalize_kernel, grid, dim3(256), 0, st, fin, descs, n, mean3[0], mean3[1],
                       mean3[2], std3[0], std3[1], std3[2], out);
    HIP_LAUNCH_CHECK();
    return UNIIR_OK;
}
