// Validation metrics on the device: SSIM over the [H,W,C] volume with an 11^3 Gaussian window (sigma 1.5) and replicate
// borders -- the reference's _ssim_3d (metrics/psnr_ssim.py:131-176), which also runs on the GPU there (conv3d .cuda()).
//
// One workgroup owns a 16x16 pixel tile x all C channels (one channel of the volume at a time).  The 11^3 window is
// separable: the channel axis (C <= 4, replicate padded by 5 either side) collapses into a C x C matrix applied while the
// haloed tile is staged into LDS, then an 11-tap pass along W and one along H.  The five filtered fields (a, b, a^2, b^2,
// ab) never leave the chip; the kernel writes one partial sum of the SSIM map per workgroup, the finish kernel folds them
// in double.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "tdr_ssim_core.h"

// (the workgroup body lives in tdr_ssim_core.h: tdr_valmetrics.hip runs the same arithmetic on the quantised bytes of a cropped image)
namespace {

using tdr_ssim::T;

struct SsimArgs {
    const float* a;
    const float* b;
    float c1, c2;
    tdr_ssim::Ssim3dParams q;
    float* partial;
};

template <int C>
struct FloatLoader {
    const float* pa; const float* pb; int W;
    __device__ __forceinline__ float a(int y, int x, int j) const { return pa[((int64_t)y * W + x) * C + j]; }
    __device__ __forceinline__ float b(int y, int x, int j) const { return pb[((int64_t)y * W + x) * C + j]; }
};

template <int C>
__global__ __launch_bounds__(256) void ssim3d_kernel(SsimArgs p) {
    const FloatLoader<C> ld{p.a, p.b, p.q.W};
    tdr_ssim::ssim3d_tile<C>(p.q, p.c1, p.c2, ld, p.partial);
}

__global__ __launch_bounds__(256) void ssim_finish_kernel(const float* partial, int n, double inv_count, float* out) {
    const float v = tdr_ssim::ssim3d_fold(partial, n, inv_count);
    if (threadIdx.x == 0) out[0] = v;
}

}  // namespace

extern "C" int64_t tdr_ssim3d_ws_floats(int H, int W) {
    return (int64_t)((H + T - 1) / T) * ((W + T - 1) / T);
}

extern "C" int tdr_ssim3d(const float* img1, const float* img2, int H, int W, int C, float max_value, float* ws, float* out,
                          void* stream) {
    if (!img1 || !img2 || !ws || !out || H < 1 || W < 1 || C < 1 || C > 4) return 1;
    SsimArgs p;
    p.a = img1; p.b = img2;
    p.c1 = tdr_ssim::ssim3d_c1(max_value);
    p.c2 = tdr_ssim::ssim3d_c2(max_value);
    tdr_ssim::ssim3d_fill(p.q, H, W, C);
    p.partial = ws;
    dim3 grid((W + T - 1) / T, (H + T - 1) / T);
    hipStream_t st = (hipStream_t)stream;
    switch (C) {
        case 1: hipLaunchKernelGGL(ssim3d_kernel<1>, grid, dim3(256), 0, st, p); break;
        case 2: hipLaunchKernelGGL(ssim3d_kernel<2>, grid, dim3(256), 0, st, p); break;
        case 3: hipLaunchKernelGGL(ssim3d_kernel<3>, grid, dim3(256), 0, st, p); break;
        default: hipLaunchKernelGGL(ssim3d_kernel<4>, grid, dim3(256), 0, st, p); break;
    }
    hipLaunchKernelGGL(ssim_finish_kernel, dim3(1), dim3(256), 0, st, ws, (int)(grid.x * grid.y),
                       1.0 / ((double)H * W * C), out);
    return hipGetLastError() == hipSuccess ? 0 : 2;
}
