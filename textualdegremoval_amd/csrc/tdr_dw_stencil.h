// The register-window row access of the depthwise 3x3 stencils (tdr_dwsg.hip; the modulated forward stencil of tdr_dyn_infer.hip): a
// thread owns a 4-column strip, a row arrives as one float4 per plane and its x-1 / x+4 neighbours from the adjacent lanes.  With the
// launch geometry of those stencils and the finish of their SCA pool partials.  Kernels and helpers have internal linkage per unit.
#pragma once
#include "tdr_common.h"

namespace {

struct Row6 { float v[6]; };

// one row of the 4-column strip with its two horizontal neighbours; zero outside the image
__device__ __forceinline__ Row6 fetch_row(const float* __restrict__ plane, int y, int x0, int H, int W, bool active,
                                          bool left_lane, bool right_lane) {
    const bool rok = active && y >= 0 && y < H;
    const float* row = plane + (long)min(max(y, 0), H - 1) * W;
    f32x4 m = {0.f, 0.f, 0.f, 0.f};
    if (rok) m = *reinterpret_cast<const f32x4*>(row + x0);
    float l = __shfl_up(m[3], 1, 64), r = __shfl_down(m[0], 1, 64);
    if (!left_lane) l = (rok && x0 > 0) ? row[x0 - 1] : 0.f;
    if (!right_lane) r = (rok && x0 + 4 < W) ? row[x0 + 4] : 0.f;
    Row6 o;
    o.v[0] = l; o.v[1] = m[0]; o.v[2] = m[1]; o.v[3] = m[2]; o.v[4] = m[3]; o.v[5] = r;
    return o;
}

// fetch_row in two halves, so that a row can be requested one loop iteration before its neighbours are exchanged
struct RawRow { f32x4 m; float le, re; };
__device__ __forceinline__ RawRow load_raw(const float* __restrict__ plane, int y, int x0, int H, int W, bool active,
                                           bool left_lane, bool right_lane) {
    RawRow r;
    r.m = f32x4{0.f, 0.f, 0.f, 0.f};
    r.le = 0.f; r.re = 0.f;
    if (active && y >= 0 && y < H) {
        const float* row = plane + (long)y * W;
        r.m = *reinterpret_cast<const f32x4*>(row + x0);
        if (!left_lane && x0 > 0) r.le = row[x0 - 1];
        if (!right_lane && x0 + 4 < W) r.re = row[x0 + 4];
    }
    return r;
}
__device__ __forceinline__ Row6 finish_row(const RawRow& r, bool left_lane, bool right_lane) {
    float l = __shfl_up(r.m[3], 1, 64), rr = __shfl_down(r.m[0], 1, 64);
    if (!left_lane) l = r.le;
    if (!right_lane) rr = r.re;
    Row6 o;
    o.v[0] = l; o.v[1] = r.m[0]; o.v[2] = r.m[1]; o.v[3] = r.m[2]; o.v[4] = r.m[3]; o.v[5] = rr;
    return o;
}

// pooled[i] = inv_hw * sum_k part[i][k]: the fixed-order finish of the per-block pool partials
__global__ void dw_pool_finish_kernel(const float* __restrict__ part, int NC, int nb, float inv_hw, float* __restrict__ pooled) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= NC) return;
    float s = 0.f;
    for (int k = 0; k < nb; ++k) s += part[(long)i * nb + k];
    pooled[i] = s * inv_hw;
}

struct DwGeom { int tprw_log2, rpt, ncb, nby, nb; };

// launch geometry of the forward stencils and the two-pass backward
inline DwGeom dw_geom(int H, int W) {
    DwGeom g;
    int groups = W / 4, lg = 0;
    while ((1 << lg) < groups && lg < 8) ++lg;          // threads per row block: next power of two, at most 256
    g.tprw_log2 = lg;
    const int spb = 256 >> lg;                           // strips per block
    g.ncb = tdr_cdiv(groups, 1 << lg);
    int rpt = tdr_cdiv(H, spb);                          // rows per thread: up to 8, fewer on small maps (more blocks)
    if (rpt > 8) rpt = 8;
    if (rpt < 1) rpt = 1;
    g.rpt = rpt;
    g.nby = tdr_cdiv(H, spb * rpt);
    g.nb = g.ncb * g.nby;
    return g;
}

}  // namespace
