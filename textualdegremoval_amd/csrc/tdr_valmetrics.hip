// Validation metrics without the host trip: PSNR and SSIM of `use_image: true` validation (models/image_restoration_ref_model.py:
// tensor2img -> calculate_psnr / calculate_ssim per image) from device tensors, for all N images of a call.
//
//   stage  : one thread per 4 pixels of the cropped region.  Quantises a float source as tdr_planes_to_img_u8 does (a byte source is
//            taken as it is), keeps the cropped bytes [N][h][w][C] in the workspace for the SSIM kernels, forms the Y planes, and
//            reduces per workgroup: the squared byte error (integers), the largest byte of pred, the squared Y error (double).
//   fold   : one workgroup per image folds those partials in a fixed order -> out[n][0 .. 5] and the per-image maximum the
//            SSIM-3D constants hang on (the host rule `1 if img.max() <= 1 else 255`).
//   ssim3d : the workgroup body of tdr_ssim3d (tdr_ssim_core.h) on the cropped bytes, blockIdx.z the image.
//   ssim_y : the workgroup body of tdr_ssim_y64 on Y planes formed from the cropped bytes while staging.
//   finish : folds the SSIM partials per image in the order of the plain kernels' finish.
// Everything is a two-stage reduction in a fixed order: no atomics, the same call gives the same bits.
#include "tdr_common.h"
#include "tdr_ssim_core.h"
#include "../../include/tdr.h"

namespace {

// what_mask (include/tdr.h)
constexpr int TDR_VALM_PSNR = 1, TDR_VALM_SSIM = 2, TDR_VALM_PSNR_Y = 4, TDR_VALM_SSIM_Y = 8, TDR_VALM_Y_PLANES = 16, TDR_VALM_ALL = 31;

constexpr int PX = 4;                   // pixels per thread of the stage kernel
constexpr int WG_PX = 256 * PX;          // pixels per workgroup

struct U8Table { float v[256]; };

struct ValSrc {
    const float* f;                      // float32 planes, strides in elements ...
    const uint8_t* u;                    // ... or dense uint8 [N][H][W][C]
    int64_t sn, sc, sr;
};

struct StageArgs {
    ValSrc a, b;
    int H, W, crop, h, w, swap;
    int keep_bytes, want_y;
    uint8_t* qa; uint8_t* qb;            // [N][h][w][C]
    float* ya; float* yb;                // [N][h][w] or null
    unsigned long long* s_part; int* m_part; double* y_part;   // [N][nb]
    U8Table tab;
};

__device__ __forceinline__ uint32_t to_u8(float x) {                 // tdr_planes_to_img_u8's rounding
    x = fminf(fmaxf(x, 0.f), 1.f);
    return (uint32_t)rintf(x * 255.0f);
}

template <int C>
__device__ __forceinline__ void load_px(const ValSrc& s, int n, int H, int W, int y, int x, int swap, uint32_t* q) {
    if (s.u) {
        const uint8_t* p = s.u + (((int64_t)n * H + y) * W + x) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = p[c];
    } else {
        const float* p = s.f + (int64_t)n * s.sn + (int64_t)y * s.sr + x;
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = to_u8(p[(int64_t)((C == 3 && swap) ? 2 - c : c) * s.sc]);
    }
}

// metrics.to_y_channel on one pixel: float32(u) / 255 from the table, the BT.601 dot product in double, term by term and unfused
// (numpy's order), one division, one float32 rounding, one float32 product.  Plain operators with contraction off: HIP's __dmul_rn /
// __dadd_rn are inline operators that carry the translation unit's contraction and fuse with each other.
template <int C>
__device__ __forceinline__ float y_of(const uint32_t* q, const float* lut) {
#pragma clang fp contract(off)
    if (C == 1) return lut[q[0]] * 255.0f;
    const double f0 = (double)lut[q[0]], f1 = (double)lut[q[C == 1 ? 0 : 1]], f2 = (double)lut[q[C == 1 ? 0 : 2]];
    const double p0 = f0 * 24.966, p1 = f1 * 128.553, p2 = f2 * 65.481;
    const double d = (((p0 + p1) + p2) + 16.0) / 255.0;
    return (float)d * 255.0f;
}

__device__ __forceinline__ double sq_acc(double s, float a, float b) {
#pragma clang fp contract(off)
    const double d = (double)a - (double)b;
    const double dd = d * d;
    return s + dd;
}

template <int C>
__global__ __launch_bounds__(256) void val_stage_kernel(StageArgs p) {
    __shared__ float lut[256];
    __shared__ unsigned long long red_s[256];
    __shared__ int red_m[256];
    __shared__ double red_y[256];
    const int tid = threadIdx.x, n = blockIdx.z;
    lut[tid] = p.tab.v[tid];
    __syncthreads();
    const int64_t hw = (int64_t)p.h * p.w;
    uint32_t s = 0u;
    int mx = 0;
    double sy = 0.0;
#pragma unroll
    for (int k = 0; k < PX; ++k) {
        const int64_t i = (int64_t)blockIdx.x * WG_PX + k * 256 + tid;
        if (i < hw) {
            const int y = (int)(i / p.w), x = (int)(i - (int64_t)y * p.w);
            uint32_t qa[C], qb[C];
            load_px<C>(p.a, n, p.H, p.W, y + p.crop, x + p.crop, p.swap, qa);
            load_px<C>(p.b, n, p.H, p.W, y + p.crop, x + p.crop, p.swap, qb);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int d = (int)qa[c] - (int)qb[c];
                s += (uint32_t)(d * d);
                mx = max(mx, (int)qa[c]);
            }
            const int64_t o = (int64_t)n * hw + i;
            if (p.keep_bytes) {
#pragma unroll
                for (int c = 0; c < C; ++c) { p.qa[o * C + c] = (uint8_t)qa[c]; p.qb[o * C + c] = (uint8_t)qb[c]; }
            }
            if (p.want_y) {
                const float ya = y_of<C>(qa, lut), yb = y_of<C>(qb, lut);
                if (p.ya) p.ya[o] = ya;
                if (p.yb) p.yb[o] = yb;
                sy = sq_acc(sy, ya, yb);
            }
        }
    }
    red_s[tid] = s; red_m[tid] = mx; red_y[tid] = sy;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {                       // fixed-order tree
        if (tid < o) {
            red_s[tid] += red_s[tid + o];
            red_m[tid] = max(red_m[tid], red_m[tid + o]);
            red_y[tid] = red_y[tid] + red_y[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const int64_t o = (int64_t)n * gridDim.x + blockIdx.x;
        p.s_part[o] = red_s[0]; p.m_part[o] = red_m[0]; p.y_part[o] = red_y[0];
    }
}

// out[n] = {S, max byte of pred, elements, 0 (SSIM), Y squared error, Y elements, 0 (SSIM-Y), 0}
__global__ __launch_bounds__(256) void val_fold_kernel(const unsigned long long* __restrict__ s_part, const int* __restrict__ m_part,
                                                       const double* __restrict__ y_part, int nb, double count, double count_y,
                                                       int* __restrict__ maxv, double* __restrict__ out) {
    __shared__ unsigned long long red_s[256];
    __shared__ int red_m[256];
    __shared__ double red_y[256];
    const int tid = threadIdx.x, n = blockIdx.x;
    unsigned long long s = 0ull;
    int mx = 0;
    double sy = 0.0;
    for (int i = tid; i < nb; i += 256) {
        const int64_t o = (int64_t)n * nb + i;
        s += s_part[o]; mx = max(mx, m_part[o]); sy += y_part[o];
    }
    red_s[tid] = s; red_m[tid] = mx; red_y[tid] = sy;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            red_s[tid] += red_s[tid + o];
            red_m[tid] = max(red_m[tid], red_m[tid + o]);
            red_y[tid] = red_y[tid] + red_y[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        maxv[n] = red_m[0];
        double* o = out + (int64_t)n * 8;
        o[0] = (double)red_s[0]; o[1] = (double)red_m[0]; o[2] = count; o[3] = 0.0;
        o[4] = red_y[0]; o[5] = count_y; o[6] = 0.0; o[7] = 0.0;
    }
}

template <int C>
struct ByteLoader {
    const uint8_t* pa; const uint8_t* pb; int W;
    __device__ __forceinline__ float a(int y, int x, int j) const { return (float)pa[((int64_t)y * W + x) * C + j]; }
    __device__ __forceinline__ float b(int y, int x, int j) const { return (float)pb[((int64_t)y * W + x) * C + j]; }
};

struct Ssim3dConsts { float c1_1, c2_1, c1_255, c2_255; };

template <int C>
__global__ __launch_bounds__(256) void val_ssim3d_kernel(tdr_ssim::Ssim3dParams p, Ssim3dConsts k, const uint8_t* __restrict__ qa,
                                                         const uint8_t* __restrict__ qb, const int* __restrict__ maxv,
                                                         float* __restrict__ partial) {
    const int n = blockIdx.z;
    const int64_t img = (int64_t)n * p.H * p.W * C;
    const bool unit = maxv[n] <= 1;                          // max_value = 1 if img.max() <= 1 else 255
    const ByteLoader<C> ld{qa + img, qb + img, p.W};
    tdr_ssim::ssim3d_tile<C>(p, unit ? k.c1_1 : k.c1_255, unit ? k.c2_1 : k.c2_255, ld, partial + (int64_t)n * gridDim.x * gridDim.y);
}

template <int C>
struct YLoader {
    const uint8_t* pa; const uint8_t* pb; int W; const float* lut;
    __device__ __forceinline__ float y(const uint8_t* p, int yy, int x) const {
        const uint8_t* s = p + ((int64_t)yy * W + x) * C;
        uint32_t q[C];
#pragma unroll
        for (int c = 0; c < C; ++c) q[c] = s[c];
        return y_of<C>(q, lut);
    }
    __device__ __forceinline__ float a(int yy, int x) const { return y(pa, yy, x); }
    __device__ __forceinline__ float b(int yy, int x) const { return y(pb, yy, x); }
};

template <int C>
__global__ __launch_bounds__(256) void val_ssim_y_kernel(tdr_ssim::SsimYParams p, const uint8_t* __restrict__ qa,
                                                         const uint8_t* __restrict__ qb, double* __restrict__ partial, U8Table tab) {
    __shared__ float lut[256];
    lut[threadIdx.x] = tab.v[threadIdx.x];
    __syncthreads();
    const int n = blockIdx.z;
    const int64_t img = (int64_t)n * p.H * p.W * C;
    const YLoader<C> ld{qa + img, qb + img, p.W, lut};
    tdr_ssim::ssim_y64_tile(p, ld, partial + (int64_t)n * gridDim.x * gridDim.y);
}

__global__ __launch_bounds__(256) void val_finish_kernel(const float* __restrict__ p3, const double* __restrict__ py, int nt,
                                                         double inv3, double invy, double* __restrict__ out) {
    const int n = blockIdx.x;
    if (p3) {
        const float v = tdr_ssim::ssim3d_fold(p3 + (int64_t)n * nt, nt, inv3);
        if (threadIdx.x == 0) out[(int64_t)n * 8 + 3] = (double)v;
    }
    if (py && threadIdx.x == 0) out[(int64_t)n * 8 + 6] = tdr_ssim::ssim_y64_fold(py + (int64_t)n * nt, nt, invy);
}

struct ValWs { int64_t qa, qb, s_part, y_part, m_part, maxv, p3, py, total; };

int64_t up16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// offsets in bytes for an N x H x W call of up to 3 channels, any crop (a crop only shrinks what is used)
ValWs val_ws(int N, int H, int W) {
    const int64_t hw = (int64_t)H * W, nb = (hw + WG_PX - 1) / WG_PX;
    const int64_t nt = (int64_t)tdr_cdiv(H, tdr_ssim::T) * tdr_cdiv(W, tdr_ssim::T);
    ValWs o;
    int64_t at = 0;
    o.qa = at; at += up16(N * hw * 3);
    o.qb = at; at += up16(N * hw * 3);
    o.s_part = at; at += up16(N * nb * 8);
    o.y_part = at; at += up16(N * nb * 8);
    o.m_part = at; at += up16(N * nb * 4);
    o.maxv = at; at += up16((int64_t)N * 4);
    o.p3 = at; at += up16(N * nt * 4);
    o.py = at; at += up16(N * nt * 8);
    o.total = at;
    return o;
}

const U8Table& u8_table() {
    static const U8Table tab = [] {
        U8Table t;
        for (int u = 0; u < 256; ++u) t.v[u] = (float)u / 255.0f;
        return t;
    }();
    return tab;
}

}  // namespace

extern "C" int64_t tdr_val_metrics_ws_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return 0;
    return val_ws(N, H, W).total;
}

extern "C" int tdr_val_metrics(const float* pred, const uint8_t* pred_u8, int64_t pred_ns, int64_t pred_cs, int64_t pred_rs,
                               const float* gt, const uint8_t* gt_u8, int64_t gt_ns, int64_t gt_cs, int64_t gt_rs, int N, int C, int H,
                               int W, int crop, int swap_rb, int what_mask, float* y_pred, float* y_gt, void* ws, double* out,
                               void* stream) {
    TDR_REQUIRE((pred != nullptr) != (pred_u8 != nullptr), "tdr_val_metrics: exactly one of pred (float32 planes) and pred_u8 (bytes)");
    TDR_REQUIRE((gt != nullptr) != (gt_u8 != nullptr), "tdr_val_metrics: exactly one of gt (float32 planes) and gt_u8 (bytes)");
    TDR_REQUIRE(ws && out, "tdr_val_metrics: null pointer (ws, out)");
    TDR_REQUIRE(what_mask > 0 && (what_mask & ~TDR_VALM_ALL) == 0, "tdr_val_metrics: what_mask 0x%x selects nothing of 0x%x", what_mask,
                TDR_VALM_ALL);
    TDR_REQUIRE(!(what_mask & TDR_VALM_Y_PLANES) || y_pred || y_gt, "tdr_val_metrics: TDR_VALM_Y_PLANES without y_pred / y_gt");
    TDR_REQUIRE(C == 1 || C == 3, "tdr_val_metrics: %d channels (1 or 3)", C);
    TDR_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0 && (int64_t)H * W <= ((int64_t)1 << 30),
                "tdr_val_metrics: bad sizes N %d (1 ... 65535), image %d x %d", N, H, W);
    TDR_REQUIRE(crop >= 0 && 2 * (int64_t)crop < H && 2 * (int64_t)crop < W, "tdr_val_metrics: crop %d leaves nothing of %d x %d", crop, H, W);
    const int h = H - 2 * crop, w = W - 2 * crop;
    const int64_t hw = (int64_t)h * w;
    const int nb = (int)((hw + WG_PX - 1) / WG_PX);
    const ValWs L = val_ws(N, H, W);
    char* base = static_cast<char*>(ws);
    const bool ssim3 = what_mask & TDR_VALM_SSIM, ssimy = what_mask & TDR_VALM_SSIM_Y;

    StageArgs p;
    p.a = ValSrc{pred, pred_u8, pred_ns, pred_cs, pred_rs};
    p.b = ValSrc{gt, gt_u8, gt_ns, gt_cs, gt_rs};
    p.H = H; p.W = W; p.crop = crop; p.h = h; p.w = w; p.swap = swap_rb ? 1 : 0;
    p.keep_bytes = ssim3 || ssimy;
    p.want_y = (what_mask & (TDR_VALM_PSNR_Y | TDR_VALM_Y_PLANES)) || y_pred || y_gt;
    p.qa = reinterpret_cast<uint8_t*>(base + L.qa); p.qb = reinterpret_cast<uint8_t*>(base + L.qb);
    p.ya = y_pred; p.yb = y_gt;
    p.s_part = reinterpret_cast<unsigned long long*>(base + L.s_part);
    p.m_part = reinterpret_cast<int*>(base + L.m_part);
    p.y_part = reinterpret_cast<double*>(base + L.y_part);
    p.tab = u8_table();
    int* maxv = reinterpret_cast<int*>(base + L.maxv);
    float* p3 = reinterpret_cast<float*>(base + L.p3);
    double* py = reinterpret_cast<double*>(base + L.py);
    hipStream_t st = (hipStream_t)stream;

    const dim3 sgrid(nb, 1, N);
    if (C == 1) hipLaunchKernelGGL(val_stage_kernel<1>, sgrid, dim3(256), 0, st, p);
    else hipLaunchKernelGGL(val_stage_kernel<3>, sgrid, dim3(256), 0, st, p);
    TDR_LAUNCH_CHECK("val_stage_kernel");
    hipLaunchKernelGGL(val_fold_kernel, dim3(N), dim3(256), 0, st, p.s_part, p.m_part, p.y_part, nb, (double)hw * C, (double)hw, maxv, out);
    TDR_LAUNCH_CHECK("val_fold_kernel");
    if (!ssim3 && !ssimy) return TDR_OK;

    const dim3 tgrid(tdr_cdiv(w, tdr_ssim::T), tdr_cdiv(h, tdr_ssim::T), N);
    const int nt = (int)(tgrid.x * tgrid.y);
    if (ssim3) {
        tdr_ssim::Ssim3dParams q;
        tdr_ssim::ssim3d_fill(q, h, w, C);
        const Ssim3dConsts k{tdr_ssim::ssim3d_c1(1.f), tdr_ssim::ssim3d_c2(1.f), tdr_ssim::ssim3d_c1(255.f), tdr_ssim::ssim3d_c2(255.f)};
        if (C == 1) hipLaunchKernelGGL(val_ssim3d_kernel<1>, tgrid, dim3(256), 0, st, q, k, p.qa, p.qb, maxv, p3);
        else hipLaunchKernelGGL(val_ssim3d_kernel<3>, tgrid, dim3(256), 0, st, q, k, p.qa, p.qb, maxv, p3);
        TDR_LAUNCH_CHECK("val_ssim3d_kernel");
    }
    if (ssimy) {
        tdr_ssim::SsimYParams q;
        tdr_ssim::ssim_y64_fill(q, h, w);
        if (C == 1) hipLaunchKernelGGL(val_ssim_y_kernel<1>, tgrid, dim3(256), 0, st, q, p.qa, p.qb, py, p.tab);
        else hipLaunchKernelGGL(val_ssim_y_kernel<3>, tgrid, dim3(256), 0, st, q, p.qa, p.qb, py, p.tab);
        TDR_LAUNCH_CHECK("val_ssim_y_kernel");
    }
    hipLaunchKernelGGL(val_finish_kernel, dim3(N), dim3(256), 0, st, ssim3 ? p3 : nullptr, ssimy ? py : nullptr, nt,
                       1.0 / ((double)h * w * C), 1.0 / ((double)h * w), out);
    TDR_LAUNCH_CHECK("val_finish_kernel");
    return TDR_OK;
}
