// Device-side image transform of the encoders' input pipeline: what upstream
// clip._transform (reached from clip_sf.py:25-26, applied per item in src/data/mbeir_dataset.py:92-100) and BLIP's eval
// transform (backbone/transform/blip_transform.py:41-48) do on CPU workers with Pillow + torchvision:
//   Image.resize((ow, oh), BICUBIC) -> centre crop n x n -> x / 255 -> (v - mean) / std -> fp32 [3][n][n]
// on a decoded RGB uint8 image that already sits in HBM.  Integer stage bit-exact with Pillow's 8-bit resample
// (22-bit fixed-point weights, horizontal pass into a uint8 intermediate, then vertical), float stage the same two IEEE
// divisions.  HBM-bound byte work: three small launches per image, only the rows / columns the crop keeps are computed.
#include <algorithm>
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
__global__ __launch_bounds__(256) void img_batch_vertical_kernel(const uniir_image_desc* __restrict__ descs,
                                                                 const uniir_image_plan* __restrict__ plans, int n,
                                                                 const unsigned char* __restrict__ ws, float m0, float m1, float m2,
                                                                 float s0, float s1, float s2, float* __restrict__ out) {
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
    hipLaunchKernelGGL(img_batch_vertical_kernel, dim3(count, (n * n + 255) / 256), dim3(256), 0, st, descs, plans, n,
                       (const unsigned char*)ws, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out);
    HIP_LAUNCH_CHECK();
    return UNIIR_OK;
}
