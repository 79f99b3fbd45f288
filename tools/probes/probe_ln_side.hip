// Probe: the LayerNorm-backward side role of gemm_wgrad_side_kernel (csrc/ln_row.h, ln_bwd_side_rows) ALONE on c compute units --
// what rate do eight waves per CU, two rows in flight each, sustain?  The fused launch needs 4.31 GB inside the weight gradient's
// time: 61 GB/s per CU on 32 CUs (c_fc pair), 51 GB/s per CU on 48 (in_proj pair) at 263 168 x 1024.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I uniir_amd/csrc tools/probes/probe_ln_side.hip -o tools/probes/probe_ln_side
//   tools/probes/probe_ln_side [rows = 263168]
// One workgroup of 512 threads with 128 KiB of dynamic LDS per CU, as in the fused launch (nothing else can become resident).
#include "ln_row.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#define CK(x)                                                                   \
    do {                                                                        \
        hipError_t e = (x);                                                     \
        if (e != hipSuccess) {                                                  \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e));              \
            return 1;                                                           \
        }                                                                       \
    } while (0)

__global__ __launch_bounds__(512, 2) void side_only(LnBwdArgs a, float* part, float* dgamma, float* dbeta, float* colsum) {
    extern __shared__ __attribute__((aligned(16))) char lds[];
    ln_bwd_side_rows<4>(a, blockIdx.x, gridDim.x, (float*)lds, part, dgamma, dbeta, colsum);
}

int main(int argc, char** argv) {
    const int rows = argc > 1 ? atoi(argv[1]) : 263168, width = 1024;
    const size_t n = (size_t)rows * width;
    float *x, *dres, *dx, *gamma, *part, *dg, *db, *cs;
    unsigned short *dy, *dxb;
    CK(hipMalloc(&x, n * 4)); CK(hipMalloc(&dres, n * 4)); CK(hipMalloc(&dx, n * 4));
    CK(hipMalloc(&dy, n * 2)); CK(hipMalloc(&dxb, n * 2));
    CK(hipMalloc(&gamma, width * 4)); CK(hipMalloc(&dg, width * 4)); CK(hipMalloc(&db, width * 4)); CK(hipMalloc(&cs, width * 4));
    CK(hipMalloc(&part, (size_t)256 * 3 * width * 4));
    std::vector<float> h(n);
    unsigned s = 12345u;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h[i] = (float)((s >> 8) & 0xffff) / 32768.0f - 1.0f; }
    CK(hipMemcpy(x, h.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dres, h.data(), n * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dy, h.data(), n * 2, hipMemcpyHostToDevice));          // arbitrary finite-or-not bf16 bit patterns: timing only
    CK(hipMemcpy(gamma, h.data(), width * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dg, 0, width * 4)); CK(hipMemset(db, 0, width * 4)); CK(hipMemset(cs, 0, width * 4));
    LnBwdArgs a = {};
    a.x = x; a.x_stride = width; a.gamma = gamma; a.dy = dy; a.dres = dres; a.dx = dx; a.dx_stride = width; a.dx_bf16 = dxb;
    a.rows = rows; a.width = width; a.eps = 1e-5f; a.colsum = 1;
    CK(hipFuncSetAttribute((const void*)side_only, hipFuncAttributeMaxDynamicSharedMemorySize, 131072));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const double bytes = 16.0 * (double)n;          // x 4 + dy 2 + dres 4 in, dx 4 + its bf16 copy 2 out
    const int cus[] = {16, 32, 48, 64, 96, 128, 256};
    for (int c : cus) {
        float best = 1e30f;
        for (int it = 0; it < 4; ++it) {
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(side_only, dim3(c), dim3(512), 131072, 0, a, part, dg, db, cs);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (it && ms < best) best = ms;
        }
        printf("side rows alone: %d x %d on %3d CUs: %.3f ms  %.2f TB/s  %.1f GB/s per CU\n", rows, width, c, best, bytes / best * 1e-9,
               bytes / best * 1e-6 / c);
    }
    CK(hipDeviceSynchronize());
    return 0;
}
