// SSIMLoss: the validation SSIM (tdr_ssim3d: 11^3 Gaussian over the [H,W,C] volume, replicate borders) as a training criterion, value and
// gradient, for N plane images [N][C][H][W].
//
//   forward : the workgroup body of tdr_ssim3d (tdr_ssim_core.h: 16 x 16 tile, 256 threads, blockIdx.z the image) on a plane loader -- the
//             same samples give the same partials, so ssim[n] carries tdr_ssim3d's bits.  When a gradient is wanted its sink also writes
//             five coefficient maps per voxel y of the volume, in UNSHIFTED statistics (neighbouring tiles shift by different constants):
//                 d = 2 mu2 A2 / (B1 B2) - 2 mu1 S / B1     the luminance part of dS/dmu1 (variances held fixed)
//                 a = dS/dE11 = -S / B2,   b = dS/dE12 = 2 A1 / (B1 B2),   mu1,   mu2
//             with A1 = 2 mu1 mu2 + C1, A2 = 2 s12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = s11 + s22 + C2, S = A1 A2 / (B1 B2).
//   finish  : one workgroup folds the partials image by image (ssim3d_fold, tdr_ssim3d's finish) and forms the loss in double.
//   backward: dS/dmu1 = d - 2 mu1 a - mu2 b, so with G^T the adjoint of the replicate-border filter
//                 G^T(dS/dmu1) + 2 pred G^T(a) + gt G^T(b)  =  G^T(d) + 2 sum_y G^T[x,y] a[y] (pred[x] - mu1[y]) + sum_y G^T[x,y] b[y] (gt[x] - mu2[y]).
//             On near-flat images a ~ 1 / C2 ~ 1100 and the plain left-hand form cancels parts of magnitude pred * a; the right-hand form
//             carries deviations only.  It stays separable once a constant c (the tile-centre sample of the channel, any constant is exact)
//             is taken out: (pred[x] - c) G^T(a)[x] - G^T(a (mu1 - c))[x].  A workgroup owns a 16 x 16 tile of dpred and GATHERS: it stages
//             the five maps on the 26 x 26 haloed tile (zero outside the image, the channel axis mixed by the TRANSPOSE of the C x C matrix
//             on the way in), then an adjoint 11-tap pass along W and one along H.  The adjoint of a replicate border is the plain
//             correlation plus two folds: the taps that rows 0..4 spend above row 0 come back to row 0, those that the last five rows
//             spend below row L-1 come back to row L-1 (for L = 1 both land on the one row).  The folds read only rows inside the halo of
//             the tile that owns the border, so there are no atomics and the same call gives the same bits.
#include "tdr_common.h"
#include "tdr_ssim_core.h"
#include "../../include/tdr.h"

namespace {

using tdr_ssim::E;
using tdr_ssim::NF;
using tdr_ssim::R;
using tdr_ssim::T;

template <int C>
struct PlaneLoader {
    const float* pa; const float* pb; int H, W;
    __device__ __forceinline__ float a(int y, int x, int j) const { return pa[((int64_t)j * H + y) * W + x]; }
    __device__ __forceinline__ float b(int y, int x, int j) const { return pb[((int64_t)j * H + y) * W + x]; }
};

// coefficient maps: field f of channel k of this image at coef[f * fs + (k * H + y) * W + x], f = 0 .. 4 (d, a, b, mu1, mu2)
struct CoefSink {
    float* coef; int64_t fs; int H, W; float c1, c2;
    __device__ __forceinline__ void operator()(int k, int y, int x, float mu1, float mu2, float s11, float s22, float s12) const {
        if (!coef) return;
        const float a1 = 2.f * (mu1 * mu2) + c1, a2 = 2.f * s12 + c2, b1 = mu1 * mu1 + mu2 * mu2 + c1, b2 = s11 + s22 + c2;
        const float r = 1.f / (b1 * b2);
        const float S = (a1 * a2) * r;
        float* o = coef + ((int64_t)k * H + y) * W + x;
        o[0] = 2.f * (mu2 * (a2 * r) - mu1 * (S / b1));
        o[fs] = -(S / b2);
        o[2 * fs] = 2.f * (a1 * r);
        o[3 * fs] = mu1;
        o[4 * fs] = mu2;
    }
};

struct FwdArgs {
    const float* pred; const float* gt;
    float c1, c2;
    tdr_ssim::Ssim3dParams q;
    float* partial;                      // [N][tiles]
    float* coef; int64_t fs;             // [5][N][C][H][W] or null
};

template <int C>
__global__ __launch_bounds__(256) void ssim_loss_fwd_kernel(FwdArgs p) {
    const int n = blockIdx.z;
    const int64_t img = (int64_t)n * C * p.q.H * p.q.W;
    const PlaneLoader<C> ld{p.pred + img, p.gt + img, p.q.H, p.q.W};
    const CoefSink sink{p.coef ? p.coef + img : nullptr, p.fs, p.q.H, p.q.W, p.c1, p.c2};
    tdr_ssim::ssim3d_tile_sink<C>(p.q, p.c1, p.c2, ld, p.partial + (int64_t)n * gridDim.x * gridDim.y, sink);
}

// ssim[n] = tdr_ssim3d's fold of image n; loss = float32(double(w) * (1.0 - (sum_n double(ssim[n])) / N)), ascending n
__global__ __launch_bounds__(256) void ssim_loss_finish_kernel(const float* __restrict__ partial, int nt, int N, double inv_count, float w,
                                                               float* __restrict__ ssim, float* __restrict__ loss) {
#pragma clang fp contract(off)
    double acc = 0.0;
    for (int n = 0; n < N; ++n) {
        const float v = tdr_ssim::ssim3d_fold(partial + (int64_t)n * nt, nt, inv_count);
        if (threadIdx.x == 0) ssim[n] = v;
        acc += (double)v;
        __syncthreads();                 // the fold's shared words are reused by the next image
    }
    if (threadIdx.x == 0) {
        const double mean = acc / (double)N;
        loss[0] = (float)((double)w * (1.0 - mean));
    }
}

struct BwdArgs {
    const float* pred; const float* gt; const float* coef; int64_t fs;
    float* dpred;
    const TdrStepGuard* guard;
    float base, gscale;                  // -w / (N H W C); the host part of the loss scale
    int accumulate, H, W;
    float g[11], cum[5];                 // window; cum[t] = g[0] + ... + g[4 - t], the mass row t of a border spends outside the image
    float mc[16];
};

// one float32 product and, when accumulating, one float32 add: neither may fuse with what feeds it
__device__ __forceinline__ float scaled_term(float coef, float x, float old, int accumulate) {
#pragma clang fp contract(off)
    const float t = coef * x;
    return accumulate ? old + t : t;
}

// the adjoint 11-tap pass at position `pos` of an axis of length L: s(i), i = 0 .. 25, is the haloed line with s(i) at axis position
// pos - at + i - R, zero outside [0, L); `at` is the position inside the tile
template <class Line>
__device__ __forceinline__ float adjoint_taps(const BwdArgs& p, int pos, int at, int L, const Line& s) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 11; ++j) acc += p.g[10 - j] * s(at + j);
    if (pos == 0) {                      // this tile starts at 0: rows 0 .. 4 sit at 5 .. 9
#pragma unroll
        for (int t = 0; t < R; ++t) acc += p.cum[t] * s(at + R + t);
    }
    if (pos == L - 1) {                  // rows L-1 .. L-5 sit at at+5 .. at+1
#pragma unroll
        for (int t = 0; t < R; ++t) acc += p.cum[t] * s(at + R - t);
    }
    return acc;
}

template <int C>
__global__ __launch_bounds__(256) void ssim_loss_bwd_kernel(BwdArgs p) {
    __shared__ float s0[NF][E][E + 1];
    __shared__ float s1[NF][E][T + 1];
    const int tid = threadIdx.x, n = blockIdx.z;
    const int x0 = blockIdx.x * T, y0 = blockIdx.y * T;
    const int ty = tid >> 4, tx = tid & 15;
    const int64_t hw = (int64_t)p.H * p.W, img = (int64_t)n * C * hw;
    float gscale = p.gscale;
    if (p.guard) gscale *= p.guard->scale;             // powers of two: exact
    const float coef = p.base * gscale;
    const int yc = min(y0 + T / 2, p.H - 1), xc = min(x0 + T / 2, p.W - 1);
    for (int j = 0; j < C; ++j) {                      // channel of dpred
        const float* pj = p.pred + img + j * hw;
        const float* gj = p.gt + img + j * hw;
        const float ca = pj[(int64_t)yc * p.W + xc], cb = gj[(int64_t)yc * p.W + xc];
        for (int i = tid; i < E * E; i += 256) {
            const int r = i / E, c = i - r * E;
            const int y = y0 + r - R, x = x0 + c - R;
            float acc[NF] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (y >= 0 && y < p.H && x >= 0 && x < p.W) {
                const float* q = p.coef + img + (int64_t)y * p.W + x;
#pragma unroll
                for (int k = 0; k < C; ++k) {
                    const float* qk = q + k * hw;
                    const float d = qk[0], a = qk[p.fs], b = qk[2 * p.fs], m1 = qk[3 * p.fs], m2 = qk[4 * p.fs], m = p.mc[k * 4 + j];
                    acc[0] += m * d; acc[1] += m * a; acc[2] += m * (a * (m1 - ca)); acc[3] += m * b; acc[4] += m * (b * (m2 - cb));
                }
            }
#pragma unroll
            for (int f = 0; f < NF; ++f) s0[f][r][c] = acc[f];
        }
        __syncthreads();
        for (int i = tid; i < NF * E * T; i += 256) {    // along W
            const int f = i / (E * T), rem = i - f * (E * T), r = rem / T, x = rem - r * T;
            s1[f][r][x] = adjoint_taps(p, x0 + x, x, p.W, [&](int c) { return s0[f][r][c]; });
        }
        __syncthreads();
        if (y0 + ty < p.H && x0 + tx < p.W) {            // along H, then the three terms
            float v[NF];
#pragma unroll
            for (int f = 0; f < NF; ++f) v[f] = adjoint_taps(p, y0 + ty, ty, p.H, [&](int r) { return s1[f][r][tx]; });
            const int64_t o = (int64_t)(y0 + ty) * p.W + x0 + tx;
            const float pv = pj[o] - ca, gv = gj[o] - cb;
            const float x = v[0] + 2.f * (pv * v[1] - v[2]) + (gv * v[3] - v[4]);
            float* out = p.dpred + img + j * hw + o;
            *out = scaled_term(coef, x, p.accumulate ? *out : 0.f, p.accumulate);
        }
        __syncthreads();
    }
}

struct LossWs { int64_t partial, coef, total; };

LossWs loss_ws(int N, int C, int H, int W) {
    const int64_t nt = (int64_t)tdr_cdiv(H, T) * tdr_cdiv(W, T);
    LossWs o;
    o.partial = 0;
    o.coef = ((int64_t)N * nt * 4 + 15) & ~(int64_t)15;
    o.total = o.coef + (int64_t)NF * N * C * H * W * 4;
    return o;
}

}  // namespace

extern "C" int64_t tdr_ssim_loss_ws_bytes(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || C > 4 || H < 1 || W < 1) return 0;
    return loss_ws(N, C, H, W).total;
}

extern "C" int tdr_ssim_loss(const float* pred, const float* target, int N, int C, int H, int W, float max_value, float loss_weight,
                             float grad_scale, const TdrStepGuard* guard, int accumulate, float* loss, float* ssim, float* dpred, void* ws,
                             void* stream) {
    TDR_REQUIRE(pred && target && loss && ssim && ws, "tdr_ssim_loss: null pointer (pred, target, loss, ssim, ws)");
    TDR_REQUIRE(C >= 1 && C <= 4, "tdr_ssim_loss: %d channels (1 ... 4)", C);
    TDR_REQUIRE(N >= 1 && N <= 65535 && H >= 1 && W >= 1, "tdr_ssim_loss: bad sizes N %d (1 ... 65535), image %d x %d", N, H, W);
    const LossWs L = loss_ws(N, C, H, W);
    char* base = static_cast<char*>(ws);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(tdr_cdiv(W, T), tdr_cdiv(H, T), N);
    const int nt = (int)(grid.x * grid.y);
    const int64_t fs = (int64_t)N * C * H * W;

    FwdArgs f;
    f.pred = pred; f.gt = target;
    f.c1 = tdr_ssim::ssim3d_c1(max_value); f.c2 = tdr_ssim::ssim3d_c2(max_value);
    tdr_ssim::ssim3d_fill(f.q, H, W, C);
    f.partial = reinterpret_cast<float*>(base + L.partial);
    f.coef = dpred ? reinterpret_cast<float*>(base + L.coef) : nullptr;
    f.fs = fs;
    switch (C) {
        case 1: hipLaunchKernelGGL(ssim_loss_fwd_kernel<1>, grid, dim3(256), 0, st, f); break;
        case 2: hipLaunchKernelGGL(ssim_loss_fwd_kernel<2>, grid, dim3(256), 0, st, f); break;
        case 3: hipLaunchKernelGGL(ssim_loss_fwd_kernel<3>, grid, dim3(256), 0, st, f); break;
        default: hipLaunchKernelGGL(ssim_loss_fwd_kernel<4>, grid, dim3(256), 0, st, f); break;
    }
    TDR_LAUNCH_CHECK("ssim_loss_fwd_kernel");
    hipLaunchKernelGGL(ssim_loss_finish_kernel, dim3(1), dim3(256), 0, st, f.partial, nt, N, 1.0 / ((double)H * W * C), loss_weight, ssim,
                       loss);
    TDR_LAUNCH_CHECK("ssim_loss_finish_kernel");
    if (!dpred) return TDR_OK;

    BwdArgs b;
    b.pred = pred; b.gt = target; b.coef = f.coef; b.fs = fs;
    b.dpred = dpred;
    b.guard = guard;
    b.base = (float)(-(double)loss_weight / ((double)N * H * W * C));
    b.gscale = grad_scale;
    b.accumulate = accumulate ? 1 : 0;
    b.H = H; b.W = W;
    double gd[11];
    tdr_ssim::gauss11(gd);
    for (int i = 0; i < 11; ++i) b.g[i] = f.q.g[i];
    for (int t = 0; t < R; ++t) {
        double s = 0.0;
        for (int k = 0; k < R - t; ++k) s += gd[k];
        b.cum[t] = (float)s;
    }
    for (int i = 0; i < 16; ++i) b.mc[i] = f.q.mc[i];
    switch (C) {
        case 1: hipLaunchKernelGGL(ssim_loss_bwd_kernel<1>, grid, dim3(256), 0, st, b); break;
        case 2: hipLaunchKernelGGL(ssim_loss_bwd_kernel<2>, grid, dim3(256), 0, st, b); break;
        case 3: hipLaunchKernelGGL(ssim_loss_bwd_kernel<3>, grid, dim3(256), 0, st, b); break;
        default: hipLaunchKernelGGL(ssim_loss_bwd_kernel<4>, grid, dim3(256), 0, st, b); break;
    }
    TDR_LAUNCH_CHECK("ssim_loss_bwd_kernel");
    return TDR_OK;
}
