// Forward-only NAFBlock_DynamicFusion in three launches (models/archs/network_nafnet_guided_diffir_arch.py:350-375, inference):
//   tdr_dyn_head_infer   t1  = conv1(norm1(x a0 + b0))                               naf_head_fwd_kernel<C, false, SCH, MOD = true>
//   tdr_dyn_dwsg_fwd     g   = u[:c] u[c:], u = (dw3x3(t1) + bias) a1 + b1 ; SCA pool partials of g            (stencil, below)
//   tdr_dyn_tail_infer   out = conv3 -> beta residual -> norm2 -> conv4 -> (. a2 + b2) -> gate -> conv5 -> gamma residual
//                                                                                    naf_tail_fwd_kernel<C, false, SCH, MOD = true>
// a*, b*: per-(image, channel) rows of the projection output (dynfusion_engine.ProjTable).  Nothing a backward pass would read is
// written: xn, mu, rs, d2, y, yn, t4 and the gate h stay on the chip.
// The chains are the MOD = true instantiations of the kernels in tdr_nafblock_chain.h, in a translation unit of their own like the plain
// forward-only ones (tdr_nafblock_infer.hip); the row access, geometry and pool finish of the stencil are tdr_dw_stencil.h.
#include "tdr_nafblock_chain.h"
#include "tdr_dw_stencil.h"

namespace {

static int dyn_check_common(const char* fn, int N, int C, int HW, int w_fmt) {
    TDR_REQUIRE(naf_chain_supported(C, HW), "%s: needs C in {32, 64, 128, 256} and HW %% 64 == 0 (got C=%d HW=%d)", fn, C, HW);
    TDR_REQUIRE(N >= 1 && N <= 16, "%s: 1 <= N <= 16 images per call (got %d)", fn, N);
    TDR_REQUIRE(w_fmt == 2 || w_fmt == 1, "%s: weights must be packed with tdr_pack_weights_hx2 / _bx3 (mode FWD)", fn);
    return TDR_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// depthwise 3x3 (+ bias) -> u = dw a1 + b1 on both halves -> g = u[:c] u[c:] -> pool partials: the forward stencil of tdr_dwsg.hip
// (a thread owns a 4-column strip and walks its rows with a 3-row register window; neighbours by lane shuffles) with the modulation
// applied where the filtered value sits in a register.  d2 = dw(t1) is never written.
// ---------------------------------------------------------------------------------------------------------------
struct DynDwArgs {
    const float* t;      // [N][2C][H][W]
    const float* w;      // [2C][9]
    const float* b;      // [2C]
    const float *ma, *mb; long m_ns;      // [N][2C] rows
    float* g;            // [N][C][H][W]
    float* part;         // [N*C][nb] pool partials, or pooled [N*C] itself when one block covers a plane
    int C, H, W, tprw_log2, rpt, ncb;
    float pscale;
};

__global__ __launch_bounds__(256) void dyn_dwsg_fwd_kernel(DynDwArgs a) {
    __shared__ float red[4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int c = blockIdx.y, n = blockIdx.z, C = a.C, H = a.H, W = a.W;
    const int TPRW = 1 << a.tprw_log2;
    const int cg = tid & (TPRW - 1), strip = tid >> a.tprw_log2;
    const int bx = blockIdx.x % a.ncb, by = blockIdx.x / a.ncb;
    const int x0 = (bx * TPRW + cg) * 4;
    const int ybeg = (by * (256 >> a.tprw_log2) + strip) * a.rpt;
    const bool active = x0 < W && ybeg < H;
    // the neighbour lane holds the adjacent strip unless this is the first/last lane of the wave or of the row block
    const bool left_lane = lane != 0 && cg != 0;
    const bool right_lane = lane != 63 && cg != TPRW - 1;
    const long HW = (long)H * W;
    const float* p1 = a.t + ((long)n * 2 * C + c) * HW;
    const float* p2 = a.t + ((long)n * 2 * C + c + C) * HW;
    float w1[9], w2[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        w1[i] = a.w[c * 9 + i];
        w2[i] = a.w[(c + C) * 9 + i];
    }
    const float b1 = a.b[c], b2 = a.b[c + C];
    const float s1 = a.ma[(long)n * a.m_ns + c], s2 = a.ma[(long)n * a.m_ns + c + C];
    const float t1 = a.mb[(long)n * a.m_ns + c], t2 = a.mb[(long)n * a.m_ns + c + C];
    float acc = 0.f;

    Row6 r1[3], r2[3];
    r1[0] = fetch_row(p1, ybeg - 1, x0, H, W, active, left_lane, right_lane);
    r2[0] = fetch_row(p2, ybeg - 1, x0, H, W, active, left_lane, right_lane);
    r1[1] = fetch_row(p1, ybeg, x0, H, W, active, left_lane, right_lane);
    r2[1] = fetch_row(p2, ybeg, x0, H, W, active, left_lane, right_lane);
    for (int i = 0; i < a.rpt; ++i) {
        const int y = ybeg + i;
        r1[2] = fetch_row(p1, y + 1, x0, H, W, active, left_lane, right_lane);     // uniform trip count: shuffles stay converged
        r2[2] = fetch_row(p2, y + 1, x0, H, W, active, left_lane, right_lane);
        float o1[4] = {b1, b1, b1, b1}, o2[4] = {b2, b2, b2, b2};
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o1[e] += w1[ky * 3 + kx] * r1[ky].v[e + kx];
                    o2[e] += w2[ky * 3 + kx] * r2[ky].v[e + kx];
                }
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __builtin_fmaf(o1[e], s1, t1) * __builtin_fmaf(o2[e], s2, t2);
        if (active && y < H) {
            *reinterpret_cast<f32x4*>(a.g + ((long)n * C + c) * HW + (long)y * W + x0) = o;
            acc += (o[0] + o[1]) + (o[2] + o[3]);
        }
        r1[0] = r1[1]; r1[1] = r1[2];
        r2[0] = r2[1]; r2[1] = r2[2];
    }
    const float s = wave_sum(acc);
    if (lane == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) a.part[((long)n * C + c) * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + (red[2] + red[3])) * a.pscale;
}

}  // namespace

extern "C" int tdr_dyn_head_infer(const TdrDynHeadDesc* d, void* stream) {
    const char* fn = "tdr_dyn_head_infer";
    TDR_REQUIRE(d && d->x && d->a0 && d->b0 && d->lnw && d->lnb && d->w1 && d->b1 && d->t1, "%s: null pointer", fn);
    if (int rc = dyn_check_common(fn, d->N, d->C, d->HW, d->w_fmt)) return rc;
    HeadFwdArgs<true> a;
    naf_head_fill(a, d);
    a.ma = d->a0; a.mb = d->b0; a.m_ns = d->ab_ns;
    const bool bx = d->w_fmt == 1;
    NAF_DISPATCH_CS(naf_head_fwd_kernel, NAF_COMMA false, NAF_COMMA true, naf_fwd_lds_bytes(d->C, bx), a, d, stream);
    TDR_LAUNCH_CHECK("naf_head_fwd_kernel<dyn infer>");
    return TDR_OK;
}

extern "C" int tdr_dyn_tail_infer(const TdrDynTailDesc* d, void* stream) {
    const char* fn = "tdr_dyn_tail_infer";
    TDR_REQUIRE(d && d->g && d->sca && d->x && d->w3 && d->w4 && d->w5 && d->b3 && d->beta && d->lnw && d->lnb && d->b4 && d->b5 &&
                    d->gamma && d->a2 && d->b2 && d->out,
                "%s: null pointer", fn);
    if (int rc = dyn_check_common(fn, d->N, d->C, d->HW, d->w_fmt)) return rc;
    TDR_REQUIRE(d->g_ns % 4 == 0 && (reinterpret_cast<uintptr_t>(d->g) & 15) == 0, "%s: g must be 16-byte aligned", fn);
    TailArgs<true> a;
    naf_tail_fill(a, d);
    a.ma = d->a2; a.mb = d->b2; a.m_ns = d->ab_ns;
    const bool bx = d->w_fmt == 1;
    NAF_DISPATCH_CS(naf_tail_fwd_kernel, NAF_COMMA false, NAF_COMMA true, naf_fwd_lds_bytes(d->C, bx), a, d, stream);
    TDR_LAUNCH_CHECK("naf_tail_fwd_kernel<dyn infer>");
    return TDR_OK;
}

extern "C" int64_t tdr_dyn_dwsg_ws_floats(int N, int C, int H, int W) {
    return (int64_t)N * C * dw_geom(H, W).nb;
}

extern "C" int tdr_dyn_dwsg_fwd(const TdrDynDwsgDesc* d, void* stream) {
    const char* fn = "tdr_dyn_dwsg_fwd";
    TDR_REQUIRE(d && d->t && d->w && d->b && d->a1 && d->b1 && d->g && d->pooled && d->ws, "%s: null pointer", fn);
    TDR_REQUIRE(d->H > 0 && d->W > 0 && (long)d->H * d->W < (1L << 31) && naf_chain_supported(d->C, d->H * d->W),
                "%s: needs C in {32, 64, 128, 256} and HW %% 64 == 0 (got C=%d H=%d W=%d)", fn, d->C, d->H, d->W);
    TDR_REQUIRE(d->N >= 1 && d->N <= 16, "%s: 1 <= N <= 16 images per call (got %d)", fn, d->N);
    TDR_REQUIRE(d->W % 4 == 0, "%s: W must be a multiple of 4 (got %d)", fn, d->W);
    TDR_REQUIRE((reinterpret_cast<uintptr_t>(d->t) & 15) == 0 && (reinterpret_cast<uintptr_t>(d->g) & 15) == 0,
                "%s: t and g must be 16-byte aligned", fn);
    hipStream_t st = (hipStream_t)stream;
    const DwGeom q = dw_geom(d->H, d->W);
    const float inv_hw = 1.0f / (float)((long)d->H * d->W);
    const bool one = q.nb == 1;      // one block per plane: the partial IS the pool sum -- no finish launch
    DynDwArgs a{d->t, d->w, d->b, d->a1, d->b1, (long)d->ab_ns, d->g, one ? d->pooled : d->ws, d->C, d->H, d->W, q.tprw_log2, q.rpt, q.ncb,
                one ? inv_hw : 1.0f};
    hipLaunchKernelGGL(dyn_dwsg_fwd_kernel, dim3(q.nb, d->C, d->N), dim3(256), 0, st, a);
    if (!one)
        hipLaunchKernelGGL(dw_pool_finish_kernel, dim3(tdr_cdiv(d->N * d->C, 256)), dim3(256), 0, st, d->ws, d->N * d->C, q.nb, inv_hw,
                           d->pooled);
    TDR_LAUNCH_CHECK("dyn_dwsg_fwd");
    return TDR_OK;
}
