// The arithmetic of the two validation SSIM kernels, written once: the 11^3-window SSIM over the [H,W,C] volume in float32
// (tdr_metrics.hip: tdr_ssim3d) and the float64 SSIM of one plane (tdr_tlsc.hip: tdr_ssim_y64).  Each is the whole body of a
// 256-thread workgroup that owns one 16 x 16 tile; where the samples come from is the `Loader`'s business -- the plain kernels
// read float images, tdr_valmetrics.hip reads the quantised bytes of a cropped image.  The same samples give the same bits:
// tap order, per-workgroup partials and the shift by the tile-centre sample are all in here.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace tdr_ssim {

constexpr int T = 16;            // tile edge
constexpr int R = 5;             // window radius
constexpr int E = T + 2 * R;     // haloed edge
constexpr int NF = 5;            // a, b, a^2, b^2, ab

struct Ssim3dParams {
    int H, W;
    float g[11];
    float mc[16];                // [c][c'] channel-axis matrix
};

// cv2.getGaussianKernel(11, 1.5): exp(-(i-5)^2 / (2 sigma^2)) normalised in double
inline void gauss11(double* gd) {
    double gs = 0.0;
    for (int i = 0; i < 11; ++i) { gd[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); gs += gd[i]; }
    for (int i = 0; i < 11; ++i) gd[i] /= gs;
}

// the window as float32 weights and the channel axis (C <= 4, replicate padded by 5 either side) collapsed into a C x C matrix
inline void ssim3d_fill(Ssim3dParams& p, int H, int W, int C) {
    p.H = H; p.W = W;
    double gd[11];
    gauss11(gd);
    for (int i = 0; i < 11; ++i) p.g[i] = (float)gd[i];
    for (int i = 0; i < 16; ++i) p.mc[i] = 0.f;
    for (int c = 0; c < C; ++c) {
        double row[4] = {0, 0, 0, 0};
        for (int k = 0; k < 11; ++k) {
            int j = c + k - 5;
            j = j < 0 ? 0 : (j > C - 1 ? C - 1 : j);
            row[j] += gd[k];
        }
        for (int j = 0; j < C; ++j) p.mc[c * 4 + j] = (float)row[j];
    }
}

inline float ssim3d_c1(float max_value) { return (0.01f * max_value) * (0.01f * max_value); }
inline float ssim3d_c2(float max_value) { return (0.03f * max_value) * (0.03f * max_value); }

// the sink of the plain kernels: nothing but the partial sums leaves the workgroup
struct NoSink {
    __device__ __forceinline__ void operator()(int, int, int, float, float, float, float, float) const {}
};

// ld.a(y, x, j) / ld.b(y, x, j): sample of channel j at pixel (y, x) of the H x W image, as a float.  Writes partial[tile].
// sink(k, y, x, mu1, mu2, s11, s22, s12) sees the statistics of every voxel of the image after its SSIM value has joined the sum: the
// UNSHIFTED means and the (shift-invariant) variances and covariance -- tdr_ssim_loss.hip turns them into the coefficient maps of the
// backward pass.  It takes no part in the sum: the same samples give the same partials under every sink.
template <int C, class Loader, class Sink>
__device__ __forceinline__ void ssim3d_tile_sink(const Ssim3dParams& p, const float c1, const float c2, const Loader& ld, float* partial,
                                                 const Sink& sink) {
    __shared__ float s0[NF][E][E + 1];
    __shared__ float s1[NF][E][T + 1];
    __shared__ float red[4];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int ty = tid >> 4, tx = tid & 15;
    float sum = 0.f;
    // Variances are differences of window means, E[x^2] - E[x]^2: on [0,255] images both terms are ~6e4 and a float32 difference
    // loses the signal on smooth regions (the reference's _ssim_cly runs in float64, metrics/psnr_ssim.py:184-222).  The window
    // weights sum to 1, so variances and the covariance are invariant under x -> x - c: every workgroup subtracts ONE constant
    // per image (its tile-centre sample) while staging and adds it back to the means -- the squares then hold local deviations only.
    const int yc = min(y0 + T / 2, p.H - 1), xc = min(x0 + T / 2, p.W - 1);
    const float ca = ld.a(yc, xc, 0), cb = ld.b(yc, xc, 0);
    for (int k = 0; k < C; ++k) {                 // output channel of the volume
        // stage: the five raw fields at replicate-clamped coordinates, channel axis mixed on the way in
        for (int i = tid; i < E * E; i += 256) {
            const int r = i / E, c = i - r * E;
            const int y = min(max(y0 + r - R, 0), p.H - 1), x = min(max(x0 + c - R, 0), p.W - 1);
            float acc[NF] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < C; ++j) {
                const float va = ld.a(y, x, j) - ca, vb = ld.b(y, x, j) - cb, m = p.mc[k * 4 + j];
                acc[0] += m * va; acc[1] += m * vb; acc[2] += m * (va * va); acc[3] += m * (vb * vb); acc[4] += m * (va * vb);
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) s0[f][r][c] = acc[f];
        }
        __syncthreads();
        // W pass
        for (int i = tid; i < NF * E * T; i += 256) {
            const int f = i / (E * T), rem = i - f * (E * T), r = rem / T, x = rem - r * T;
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < 11; ++j) acc += p.g[j] * s0[f][r][x + j];
            s1[f][r][x] = acc;
        }
        __syncthreads();
        // H pass + the SSIM map
        if (y0 + ty < p.H && x0 + tx < p.W) {
            float v[NF];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < 11; ++j) acc += p.g[j] * s1[f][ty + j][tx];
                v[f] = acc;
            }
            const float s11 = v[2] - v[0] * v[0], s22 = v[3] - v[1] * v[1], s12 = v[4] - v[0] * v[1];   // shift-invariant
            const float mu1 = v[0] + ca, mu2 = v[1] + cb;
            const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
            sum += ((2.f * m12 + c1) * (2.f * s12 + c2)) / ((m11 + m22 + c1) * (s11 + s22 + c2));
            sink(k, y0 + ty, x0 + tx, mu1, mu2, s11, s22, s12);
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

template <int C, class Loader>
__device__ __forceinline__ void ssim3d_tile(const Ssim3dParams& p, const float c1, const float c2, const Loader& ld, float* partial) {
    ssim3d_tile_sink<C>(p, c1, c2, ld, partial, NoSink{});
}

// the fold of n per-workgroup partials of ssim3d_tile by one 256-thread workgroup -> float32(sum * inv_count), valid in thread 0
__device__ __forceinline__ float ssim3d_fold(const float* partial, int n, double inv_count) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (float)((red[0] + red[1] + red[2] + red[3]) * inv_count);
}

// ---- float64 SSIM of one channel (BORDER_REPLICATE): a workgroup owns a 16 x 16 tile, stages the 26 x 26 haloed tile of both images
// as doubles, filters the five fields separably (cv2.filter2D applies the outer product window; separable evaluation differs from it
// only by double rounding), and writes one partial sum.
struct SsimYParams { int H, W; double c1, c2; double g[11]; };

inline void ssim_y64_fill(SsimYParams& p, int H, int W) {
    p.H = H; p.W = W;
    p.c1 = (0.01 * 255) * (0.01 * 255); p.c2 = (0.03 * 255) * (0.03 * 255);
    double sum = 0.0;                                 // cv2.getGaussianKernel(11, 1.5): exp(-(i - 5)^2 / (2 sigma^2)), normalised
    for (int i = 0; i < 11; ++i) { p.g[i] = exp(-(double)((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5)); sum += p.g[i]; }
    for (int i = 0; i < 11; ++i) p.g[i] /= sum;
}

// ld.a(y, x) / ld.b(y, x): the float32 sample at pixel (y, x) of the H x W plane.  Writes partial[tile].
template <class Loader>
__device__ __forceinline__ void ssim_y64_tile(const SsimYParams& p, const Loader& ld, double* partial) {
    __shared__ double s0[5][E][E + 1];
    __shared__ double s1[5][E][T + 1];
    __shared__ double red[4];
    const int tid = threadIdx.x, x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    for (int i = tid; i < E * E; i += 256) {
        const int r = i / E, c = i - r * E;
        const int gy = min(max(y0 + r - R, 0), p.H - 1), gx = min(max(x0 + c - R, 0), p.W - 1);
        const double a = (double)ld.a(gy, gx), b = (double)ld.b(gy, gx);
        s0[0][r][c] = a; s0[1][r][c] = b; s0[2][r][c] = a * a; s0[3][r][c] = b * b; s0[4][r][c] = a * b;
    }
    __syncthreads();
    for (int i = tid; i < 5 * E * T; i += 256) {          // along W
        const int f = i / (E * T), rem = i - f * (E * T), r = rem / T, c = rem - r * T;
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) v += p.g[k] * s0[f][r][c + k];
        s1[f][r][c] = v;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    double m[5];
#pragma unroll
    for (int f = 0; f < 5; ++f) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < 11; ++k) v += p.g[k] * s1[f][ty + k][tx];
        m[f] = v;
    }
    double val = 0.0;
    if (y0 + ty < p.H && x0 + tx < p.W) {
        const double mu1 = m[0], mu2 = m[1];
        const double s11 = m[2] - mu1 * mu1, s22 = m[3] - mu2 * mu2, s12 = m[4] - mu1 * mu2;
        val = ((2 * mu1 * mu2 + p.c1) * (2 * s12 + p.c2)) / ((mu1 * mu1 + mu2 * mu2 + p.c1) * (s11 + s22 + p.c2));
    }
    // fixed-order block reduction
    for (int o = 32; o > 0; o >>= 1) val += __shfl_xor(val, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = val;
    __syncthreads();
    if (tid == 0) partial[blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the serial fold of the partials of ssim_y64_tile (one thread) -> sum * inv
__device__ __forceinline__ double ssim_y64_fold(const double* __restrict__ partial, int n, double inv) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += partial[i];
    return s * inv;
}

}  // namespace tdr_ssim
