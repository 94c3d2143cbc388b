// NIQE features on the device -- metrics/niqe.py:10-139 of the reference: the normalised (MSCN) map of the Y image at two scales and, per
// 96 x 96 block (48 x 48 at the half scale), the AGGD fits of the map and of its products with four circularly shifted copies: 18 features
// per scale.  The 36 x 36 Gaussian-model tail (:140-155) stays on the host (metrics/niqe.py).
//
// Number formats follow the reference.  scipy.ndimage.convolve accumulates every output in double and casts to the input's float32, and the
// map expression of :112-117 is float32 arithmetic: niqe_mscn_kernel does exactly that, operation by operation (no contraction: an fma
// would round differently from numpy's separate multiply and add).  The block moments are sums of float32 values and of products of two
// float32 values, both exact in double, accumulated in double in a fixed order -- the reference run on the float64 copy of the same maps.
#include "tdr_common.h"
#include "../../include/tdr.h"

#pragma clang fp contract(off)

namespace {

constexpr int MT_H = 16, MT_W = 64, MR = 3, ME_H = MT_H + 2 * MR, ME_W = MT_W + 2 * MR;

// out[y][x] = (img - mu) / (sigma + 1), mu = convolve(img, window, 'nearest'), sigma = sqrt(|convolve(img^2) - mu^2|).  A workgroup owns a
// 16 x 64 tile and stages the 22 x 70 haloed tile (replicate border = mode 'nearest').  The taps run in scipy's order: row-major over the
// FLIPPED window (convolution), every product and every sum rounded to double on its own.
__global__ __launch_bounds__(256) void niqe_mscn_kernel(const float* __restrict__ img, int H, int W, const double* __restrict__ window,
                                                        float* __restrict__ out) {
    __shared__ float tile[ME_H][ME_W + 1];
    __shared__ double wf[49];
    const int tid = threadIdx.x, x0 = blockIdx.x * MT_W, y0 = blockIdx.y * MT_H;
    if (tid < 49) wf[tid] = window[48 - tid];
    for (int i = tid; i < ME_H * ME_W; i += 256) {
        const int r = i / ME_W, c = i - r * ME_W;
        const int gy = min(max(y0 + r - MR, 0), H - 1), gx = min(max(x0 + c - MR, 0), W - 1);
        tile[r][c] = img[(long)gy * W + gx];
    }
    __syncthreads();
    const int tx = tid & (MT_W - 1), ty = tid >> 6;
    for (int r = ty; r < MT_H; r += 4) {
        const int gy = y0 + r, gx = x0 + tx;
        if (gy >= H || gx >= W) continue;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const float v = tile[r + i][tx + j];
                const float v2 = v * v;                      // np.square of the float32 image
                const double w = wf[i * 7 + j];
                s1 = s1 + (double)v * w;
                s2 = s2 + (double)v2 * w;
            }
        }
        const float x = tile[r + MR][tx + MR];
        const float mu = (float)s1, ex2 = (float)s2;
        const float sigma = sqrtf(fabsf(ex2 - mu * mu));           // sqrtf and / are the correctly rounded forms (the __f*_rn intrinsics
        out[(long)gy * W + gx] = (x - mu) / (sigma + 1.0f);      // map to the native approximations)
    }
}

// cv2.resize(img / 255., (W / 2, H / 2), INTER_LINEAR) * 255. for even H, W: both bilinear weights are 0.5, applied along x and then along y
// in float32 (the products by 0.5 are exact, so the form a * 0.5 + b * 0.5 has one rounding, that of the sum).
__global__ __launch_bounds__(256) void niqe_half_kernel(const float* __restrict__ img, int Ho, int Wo, float* __restrict__ out) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= Wo || y >= Ho) return;
    const float* p = img + (long)(2 * y) * (2 * Wo) + 2 * x;
    const float a = p[0] / 255.0f, b = p[1] / 255.0f;
    const float c = p[2 * Wo] / 255.0f, d = p[2 * Wo + 1] / 255.0f;
    const float top = a * 0.5f + b * 0.5f, bot = c * 0.5f + d * 0.5f;
    out[(long)y * Wo + x] = (top * 0.5f + bot * 0.5f) * 255.0f;
}

struct NiqeFeatArgs {
    const float* map;      // normalised map of this scale [nbh * B][nbw * B]
    int W, B, nbh;         // map width, block side at this scale, blocks per column
    const double* tab;     // [4][T]: gam, r_gam, sqrt(gamma(1/gam) / gamma(3/gam)), gamma(2/gam) / gamma(1/gam)
    int T;
    double* feats;         // [nblocks][36]
    int col0;              // 0 (scale 1) or 18 (scale 2)
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup per (block, map): map 0 is the block itself, maps 1 - 4 its product with np.roll(block, s, axis=(0, 1)) for
// s = [0,1], [1,0], [1,1], [1,-1] (wrap-around inside the block).  estimate_aggd_param (:10-37) in double: six moments reduced in a fixed
// order (per-thread strided sums, xor butterflies inside a wave, the four waves through LDS), then the first-minimum search over the r_gam
// table and the closed-form rest.  An empty side divides 0 by 0 exactly as np.mean of an empty slice does: NaN, which propagates into
// rhatnorm; np.argmin of the then all-NaN distances is 0, so alpha is gam[0] and the betas / the Eq. 8 mean stay NaN.
__global__ __launch_bounds__(256) void niqe_block_features_kernel(NiqeFeatArgs p) {
    __shared__ double red[4][6];
    __shared__ double sval[4];
    __shared__ int sidx[4];
    const int tid = threadIdx.x, wave = tid >> 6, blk = blockIdx.x, m = blockIdx.y;
    const int B = p.B, bw = blk / p.nbh, bh = blk - bw * p.nbh;
    const float* base = p.map + (long)bh * B * p.W + (long)bw * B;
    const int sy = m >= 2 ? 1 : 0, sx = m == 0 ? 0 : (m == 2 ? 0 : (m == 4 ? -1 : 1));
    double cn = 0.0, sn = 0.0, cp = 0.0, sp = 0.0, sa = 0.0, sq = 0.0;
    for (int e = tid; e < B * B; e += 256) {
        const int i = e / B, j = e - i * B;
        double x = (double)base[(long)i * p.W + j];
        if (m > 0) {
            int ii = i - sy, jj = j - sx;                   // shifted[i][j] = block[(i - sy) mod B][(j - sx) mod B]
            ii += ii < 0 ? B : 0;
            jj += jj < 0 ? B : (jj >= B ? -B : 0);
            x = x * (double)base[(long)ii * p.W + jj];     // exact: two 24-bit significands
        }
        const double x2 = x * x;
        if (x < 0.0) { cn += 1.0; sn += x2; }
        if (x > 0.0) { cp += 1.0; sp += x2; }
        sa += fabs(x);
        sq += x2;
    }
    double acc[6] = {cn, sn, cp, sp, sa, sq};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        acc[k] = wave_sum_f64(acc[k]);
        if ((tid & 63) == 0) red[wave][k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    const double cnt = (double)B * (double)B;
    const double left_std = sqrt(acc[1] / acc[0]), right_std = sqrt(acc[3] / acc[2]);
    const double gammahat = left_std / right_std;
    const double mabs = acc[4] / cnt;
    const double rhat = (mabs * mabs) / (acc[5] / cnt);
    const double g2 = gammahat * gammahat;
    const double rhatnorm = (rhat * (g2 * gammahat + 1.0) * (gammahat + 1.0)) / ((g2 + 1.0) * (g2 + 1.0));

    // np.argmin((r_gam - rhatnorm)**2): the lowest index among equal minima
    const double* r_gam = p.tab + p.T;
    double best = __builtin_inf();
    int bi = 0x7fffffff;
    for (int t = tid; t < p.T; t += 256) {
        double dd = r_gam[t] - rhatnorm;
        dd = dd * dd;
        if (bi == 0x7fffffff || dd < best) { best = dd; bi = t; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov < best || (ov == best && oi < bi)) { best = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { sval[wave] = best; sidx[wave] = bi; }
    __syncthreads();
    if (tid != 0) return;
    int pos = 0;
    if (rhatnorm == rhatnorm) {                              // NaN: every distance is NaN and np.argmin answers 0
        best = sval[0]; pos = sidx[0];
        for (int w = 1; w < 4; ++w)
            if (sval[w] < best || (sval[w] == best && sidx[w] < pos)) { best = sval[w]; pos = sidx[w]; }
    }
    const double alpha = p.tab[pos], bratio = p.tab[2 * p.T + pos], mratio = p.tab[3 * p.T + pos];
    const double beta_l = left_std * bratio, beta_r = right_std * bratio;
    double* f = p.feats + (long)blk * 36 + p.col0;
    if (m == 0) {
        f[0] = alpha;
        f[1] = (beta_l + beta_r) / 2.0;
    } else {
        f += 2 + (m - 1) * 4;
        f[0] = alpha;
        f[1] = (beta_r - beta_l) * mratio;                  // Eq. 8
        f[2] = beta_l;
        f[3] = beta_r;
    }
}

}  // namespace

extern "C" int64_t tdr_niqe_ws_floats(int H, int W) { return (int64_t)H * W + 2 * (int64_t)(H / 2) * (W / 2); }

extern "C" int tdr_niqe_features(const float* y, int H, int W, int block, const double* window, const double* tables, int table_len,
                                 float* ws, double* feats_out, void* stream) {
    TDR_REQUIRE(y && window && tables && ws && feats_out, "tdr_niqe_features: null pointer");
    TDR_REQUIRE(block >= 2 && block % 2 == 0, "tdr_niqe_features: block size %d must be even and positive", block);
    TDR_REQUIRE(H >= block && W >= block && H % block == 0 && W % block == 0,
                "tdr_niqe_features: image %d x %d is not a whole number (>= 1) of %d x %d blocks", H, W, block, block);
    TDR_REQUIRE(table_len > 0, "tdr_niqe_features: empty r_gam table");
    hipStream_t st = (hipStream_t)stream;
    const int H2 = H / 2, W2 = W / 2, nbh = H / block, nbw = W / block;
    float* map1 = ws;
    float* half = map1 + (int64_t)H * W;
    float* map2 = half + (int64_t)H2 * W2;
    hipLaunchKernelGGL(niqe_mscn_kernel, dim3(tdr_cdiv(W, MT_W), tdr_cdiv(H, MT_H)), dim3(256), 0, st, y, H, W, window, map1);
    TDR_LAUNCH_CHECK("niqe_mscn_kernel");
    hipLaunchKernelGGL(niqe_half_kernel, dim3(tdr_cdiv(W2, 64), tdr_cdiv(H2, 4)), dim3(256), 0, st, y, H2, W2, half);
    TDR_LAUNCH_CHECK("niqe_half_kernel");
    hipLaunchKernelGGL(niqe_mscn_kernel, dim3(tdr_cdiv(W2, MT_W), tdr_cdiv(H2, MT_H)), dim3(256), 0, st, (const float*)half, H2, W2, window,
                       map2);
    TDR_LAUNCH_CHECK("niqe_mscn_kernel");
    NiqeFeatArgs a;
    a.tab = tables; a.T = table_len; a.feats = feats_out; a.nbh = nbh;
    a.map = map1; a.W = W; a.B = block; a.col0 = 0;
    hipLaunchKernelGGL(niqe_block_features_kernel, dim3(nbh * nbw, 5), dim3(256), 0, st, a);
    TDR_LAUNCH_CHECK("niqe_block_features_kernel");
    a.map = map2; a.W = W2; a.B = block / 2; a.col0 = 18;
    hipLaunchKernelGGL(niqe_block_features_kernel, dim3(nbh * nbw, 5), dim3(256), 0, st, a);
    TDR_LAUNCH_CHECK("niqe_block_features_kernel");
    return TDR_OK;
}
