// Text-embedding modulation of NAFNetDynamicFusion (models/archs/network_nafnet_guided_diffir_arch.py:250-275, :328-375):
// the embedding projections `kernel` / `sg1.kernel` / `sg2.kernel` (Linear(10 * 1024, ., bias=False) on the flattened k_v) of every
// block, and the per-(image, channel) affines they feed -- before norm1, and ahead of the two SimpleGates.  Every reduction has a fixed
// order (no float atomics): per-lane sequential FMA chains, then fixed butterfly / LDS trees, then fixed-order sums of partials.
#include "tdr_common.h"
#include "../../include/tdr.h"

namespace {

constexpr int PROJ_R = 8;          // rows of one projection tile (forward: one wave; weight gradient: one workgroup)

// segment table: 4 int64 words per projection weight {W, col0, rows, tile0}; tile0 = first global tile (PROJ_R rows each)
struct Seg {
    const float* W;
    long col0;
    int rows;
    long tile0;
};

__device__ __forceinline__ Seg find_seg(const long* __restrict__ tab, int nseg, long tile) {
    int lo = 0, hi = nseg - 1;               // last segment whose tile0 <= tile
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[4 * mid + 3] <= tile) lo = mid;
        else hi = mid - 1;
    }
    Seg s;
    s.W = (const float*)tab[4 * lo];
    s.col0 = tab[4 * lo + 1];
    s.rows = (int)tab[4 * lo + 2];
    s.tile0 = tab[4 * lo + 3];
    return s;
}

// fixed-order sum over a 256-thread workgroup: butterfly inside each wave, then the four wave sums in order
__device__ __forceinline__ float block_sum256(float v, float* red) {
    v = wave_sum(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[w] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- projections, forward: out[n][col0 + r] = sum_k W[r][k] kv[n][k].  One wave per PROJ_R rows: every weight element is loaded once
// for all N images (the kv rows come from L2, reused by PROJ_R rows); lane l accumulates k = 4 (l + 64 j) + e in order of j, e, then a
// butterfly over the lanes.
template <int NB>
__global__ __launch_bounds__(256) void kvproj_fwd_kernel(const long* __restrict__ tab, int nseg, long ntiles,
                                                         const float* __restrict__ kv, int N, int K, float* __restrict__ out,
                                                         long ld) {
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= ntiles) return;
    const int lane = threadIdx.x & 63;
    const Seg s = find_seg(tab, nseg, tile);
    const int r0 = (int)(tile - s.tile0) * PROJ_R;
    const int nr = min(PROJ_R, s.rows - r0);
    float acc[PROJ_R][NB];
#pragma unroll
    for (int r = 0; r < PROJ_R; ++r)
#pragma unroll
        for (int n = 0; n < NB; ++n) acc[r][n] = 0.f;
    const float* Wt = s.W + (long)r0 * K;
    for (int k = 4 * lane; k < K; k += 256) {
        f32x4 kx[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n)
            kx[n] = n < N ? *(const f32x4*)(kv + (long)n * K + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < PROJ_R; ++r) {
            if (r < nr) {
                const f32x4 w = __builtin_nontemporal_load((const f32x4*)(Wt + (long)r * K + k));
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    float a = acc[r][n];
                    a = __builtin_fmaf(w.x, kx[n].x, a);
                    a = __builtin_fmaf(w.y, kx[n].y, a);
                    a = __builtin_fmaf(w.z, kx[n].z, a);
                    a = __builtin_fmaf(w.w, kx[n].w, a);
                    acc[r][n] = a;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < PROJ_R; ++r)
#pragma unroll
        for (int n = 0; n < NB; ++n) {
            const float v = wave_sum(acc[r][n]);
            if (lane == 0 && r < nr && n < N) out[(long)n * ld + s.col0 + r0 + r] = v;
        }
}

// ---- projections, weight gradient: dW[r][k] = sum_n dk[n][col0 + r] kv[n][k] (n in order), each element written once.
// One workgroup per PROJ_R rows; thread t owns the float4 columns 4 (t + 256 j).
template <int NB>
__global__ __launch_bounds__(256) void kvproj_wgrad_kernel(const long* __restrict__ tab, const long* __restrict__ gtab, int nseg,
                                                           const float* __restrict__ kv, const float* __restrict__ dk, long ld, int N,
                                                           int K) {
    const long tile = blockIdx.x;
    const Seg s = find_seg(tab, nseg, tile);
    int lo = 0, hi = nseg - 1;                    // the same segment's gradient pointer (gtab: one word per segment)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (tab[4 * mid + 3] <= tile) lo = mid;
        else hi = mid - 1;
    }
    float* dW = (float*)gtab[lo];
    const int r0 = (int)(tile - s.tile0) * PROJ_R;
    const int nr = min(PROJ_R, s.rows - r0);
    float g[PROJ_R][NB];
#pragma unroll
    for (int r = 0; r < PROJ_R; ++r)
#pragma unroll
        for (int n = 0; n < NB; ++n) g[r][n] = (r < nr && n < N) ? dk[(long)n * ld + s.col0 + r0 + r] : 0.f;
    for (int k = 4 * threadIdx.x; k < K; k += 1024) {
        f32x4 kx[NB];
#pragma unroll
        for (int n = 0; n < NB; ++n)
            kx[n] = n < N ? *(const f32x4*)(kv + (long)n * K + k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int r = 0; r < PROJ_R; ++r) {
            if (r < nr) {
                f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int n = 0; n < NB; ++n) {
                    o.x = __builtin_fmaf(g[r][n], kx[n].x, o.x);
                    o.y = __builtin_fmaf(g[r][n], kx[n].y, o.y);
                    o.z = __builtin_fmaf(g[r][n], kx[n].z, o.z);
                    o.w = __builtin_fmaf(g[r][n], kx[n].w, o.w);
                }
                __builtin_nontemporal_store(o, (f32x4*)(dW + (long)(r0 + r) * K + k));
            }
        }
    }
}

// ---- projections, gradient of k_v, first stage: workgroup (kb, s) sums the tiles [s tpb, (s + 1) tpb) over the columns
// k in [1024 kb, 1024 kb + 1024): part[s][n][k] = sum over those rows in order of dk[n][row] W[row][k]
template <int NB>
__global__ __launch_bounds__(256) void kvproj_dkv_part_kernel(const long* __restrict__ tab, int nseg, long ntiles, int tpb,
                                                              const float* __restrict__ dk, long ld, int N, int K,
                                                              float* __restrict__ part) {
    const int k = 1024 * blockIdx.x + 4 * threadIdx.x;
    const long t0 = (long)blockIdx.y * tpb;
    const long t1 = min(ntiles, t0 + tpb);
    f32x4 acc[NB];
#pragma unroll
    for (int n = 0; n < NB; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    const bool kok = k < K;
    for (long t = t0; t < t1; ++t) {
        const Seg s = find_seg(tab, nseg, t);
        const int r0 = (int)(t - s.tile0) * PROJ_R;
        const int nr = min(PROJ_R, s.rows - r0);
        for (int r = 0; r < nr; ++r) {
            const long row = r0 + r;
            const f32x4 w = kok ? __builtin_nontemporal_load((const f32x4*)(s.W + row * K + k)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int n = 0; n < NB; ++n) {
                if (n < N) {
                    const float d = dk[(long)n * ld + s.col0 + row];
                    acc[n].x = __builtin_fmaf(d, w.x, acc[n].x);
                    acc[n].y = __builtin_fmaf(d, w.y, acc[n].y);
                    acc[n].z = __builtin_fmaf(d, w.z, acc[n].z);
                    acc[n].w = __builtin_fmaf(d, w.w, acc[n].w);
                }
            }
        }
    }
    if (!kok) return;
#pragma unroll
    for (int n = 0; n < NB; ++n)
        if (n < N) *(f32x4*)(part + ((long)blockIdx.y * N + n) * K + k) = acc[n];
}

// second stage: dkv[i] = sum_s part[s][i], s in order
__global__ __launch_bounds__(256) void kvproj_dkv_finish_kernel(const float* __restrict__ part, int S, long len,
                                                                float* __restrict__ dkv) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= len) return;
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += part[(long)s * len + i];
    dkv[i] = a;
}

// ---- LayerNorm2d of m = x a[n][c] + b[n][c] (NAFBlock_DynamicFusion.forward :353-357): the ln_fwd_generic_kernel of tdr_pointwise.hip
// with the affine applied as x is read.  mu / rstd are those of m.
__global__ __launch_bounds__(1024) void modln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                         const float* __restrict__ b, long ab_ns, const float* __restrict__ w,
                                                         const float* __restrict__ lb, float eps, int C, int HW,
                                                         float* __restrict__ y, float* __restrict__ mu, float* __restrict__ rstd) {
    __shared__ float red[16][64];
    const int lane = threadIdx.x & 63, slice = threadIdx.x >> 6;
    const int px = blockIdx.x * 64 + lane, n = blockIdx.y;
    const bool pok = px < HW;
    const float* xn = x + (long)n * C * HW + (pok ? px : HW - 1);
    const float* an = a + (long)n * ab_ns;
    const float* bn = b + (long)n * ab_ns;
    auto total = [&]() {
        float t = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += red[k][lane];
        return t;
    };
    float s = 0.f;
    for (int c = slice; c < C; c += 16) s += __builtin_fmaf(xn[(long)c * HW], an[c], bn[c]);
    red[slice][lane] = s;
    __syncthreads();
    const float mean = total() / (float)C;
    __syncthreads();
    float q = 0.f;
    for (int c = slice; c < C; c += 16) {
        const float d = __builtin_fmaf(xn[(long)c * HW], an[c], bn[c]) - mean;
        q += d * d;
    }
    red[slice][lane] = q;
    __syncthreads();
    const float rs = 1.0f / sqrtf(total() / (float)C + eps);
    if (!pok) return;
    float* yn = y + ((long)n * C) * HW + px;
    for (int c = slice; c < C; c += 16)
        yn[(long)c * HW] = (__builtin_fmaf(xn[(long)c * HW], an[c], bn[c]) - mean) * rs * w[c] + lb[c];
    if (slice == 0) {
        mu[(long)n * HW + px] = mean;
        rstd[(long)n * HW + px] = rs;
    }
}

// m = x a[n][c] + b[n][c] (the backward pass recomputes the LayerNorm input instead of keeping it)
__global__ __launch_bounds__(256) void nc_affine_kernel(const float* __restrict__ x, const float* __restrict__ a,
                                                        const float* __restrict__ b, long ab_ns, int C, int HW, long total,
                                                        float* __restrict__ y) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long plane = i / HW;
    const int n = (int)(plane / C), c = (int)(plane % C);
    y[i] = __builtin_fmaf(x[i], a[(long)n * ab_ns + c], b[(long)n * ab_ns + c]);
}

// backward of m = x a + b, one workgroup per (n, c) plane: dx = a dm (+ add), da = sum dm x, db = sum dm (fixed order)
__global__ __launch_bounds__(256) void nc_affine_bwd_kernel(const float* __restrict__ dm, const float* __restrict__ x,
                                                            const float* __restrict__ a, long ab_ns, const float* __restrict__ add,
                                                            int C, int HW, float* __restrict__ dx, float* __restrict__ da,
                                                            float* __restrict__ db, long d_ns) {
    __shared__ float red[4];
    const int n = blockIdx.x / C, c = blockIdx.x % C;
    const long base = (long)blockIdx.x * HW;
    const float av = a[(long)n * ab_ns + c];
    float sx = 0.f, s1 = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) {
        const float g = dm[base + p], xv = x[base + p];
        sx = __builtin_fmaf(g, xv, sx);
        s1 += g;
        dx[base + p] = add ? __builtin_fmaf(av, g, add[base + p]) : av * g;
    }
    sx = block_sum256(sx, red);
    s1 = block_sum256(s1, red);
    if (threadIdx.x == 0) {
        da[(long)n * d_ns + c] = sx;
        db[(long)n * d_ns + c] = s1;
    }
}

// modulated SimpleGate (SimpleGate_DynamicFusion.forward :250-275), one workgroup per (n, j < c) pair of planes of t [N][2c][HW]:
// u = t a + b over the 2c channels, g[n][j] = u[j] u[j + c]; pooled[n][j] = mean g (the SCA input after sg1) when asked for
__global__ __launch_bounds__(256) void modgate_fwd_kernel(const float* __restrict__ t, const float* __restrict__ a,
                                                          const float* __restrict__ b, long ab_ns, int c, int HW,
                                                          float* __restrict__ g, float* __restrict__ pooled) {
    __shared__ float red[4];
    const int n = blockIdx.x / c, j = blockIdx.x % c;
    const float* t1 = t + ((long)n * 2 * c + j) * HW;
    const float* t2 = t1 + (long)c * HW;
    const float a1 = a[(long)n * ab_ns + j], a2 = a[(long)n * ab_ns + c + j];
    const float b1 = b[(long)n * ab_ns + j], b2 = b[(long)n * ab_ns + c + j];
    float* gp = g + (long)blockIdx.x * HW;
    float s = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) {
        const float v = __builtin_fmaf(t1[p], a1, b1) * __builtin_fmaf(t2[p], a2, b2);
        gp[p] = v;
        s += v;
    }
    if (!pooled) return;
    s = block_sum256(s, red);
    if (threadIdx.x == 0) pooled[blockIdx.x] = s / (float)HW;
}

// its backward: d = dg (+ dgb[n][j] mul), du1 = d u2, du2 = d u1; dt = a du; da = sum du t, db = sum du per channel of 2c
__global__ __launch_bounds__(256) void modgate_bwd_kernel(const float* __restrict__ dg, const float* __restrict__ dgb, float dgb_mul,
                                                          const float* __restrict__ t, const float* __restrict__ a,
                                                          const float* __restrict__ b, long ab_ns, int c, int HW,
                                                          float* __restrict__ dt, float* __restrict__ da, float* __restrict__ db,
                                                          long d_ns) {
    __shared__ float red[4];
    const int n = blockIdx.x / c, j = blockIdx.x % c;
    const long o1 = ((long)n * 2 * c + j) * HW, o2 = o1 + (long)c * HW;
    const float a1 = a[(long)n * ab_ns + j], a2 = a[(long)n * ab_ns + c + j];
    const float b1 = b[(long)n * ab_ns + j], b2 = b[(long)n * ab_ns + c + j];
    const float* dgp = dg + (long)blockIdx.x * HW;
    const float bias = dgb ? dgb[blockIdx.x] * dgb_mul : 0.f;
    float sa1 = 0.f, sb1 = 0.f, sa2 = 0.f, sb2 = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) {
        const float d = dgp[p] + bias;
        const float x1 = t[o1 + p], x2 = t[o2 + p];
        const float u1 = __builtin_fmaf(x1, a1, b1), u2 = __builtin_fmaf(x2, a2, b2);
        const float du1 = d * u2, du2 = d * u1;
        dt[o1 + p] = a1 * du1;
        dt[o2 + p] = a2 * du2;
        sa1 = __builtin_fmaf(du1, x1, sa1);
        sb1 += du1;
        sa2 = __builtin_fmaf(du2, x2, sa2);
        sb2 += du2;
    }
    sa1 = block_sum256(sa1, red);
    sb1 = block_sum256(sb1, red);
    sa2 = block_sum256(sa2, red);
    sb2 = block_sum256(sb2, red);
    if (threadIdx.x == 0) {
        da[(long)n * d_ns + j] = sa1;
        da[(long)n * d_ns + c + j] = sa2;
        db[(long)n * d_ns + j] = sb1;
        db[(long)n * d_ns + c + j] = sb2;
    }
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
#define KVP_DISPATCH(KERNEL, N, ...)                                          \
    do {                                                                      \
        if ((N) <= 1) hipLaunchKernelGGL((KERNEL<1>), __VA_ARGS__);           \
        else if ((N) <= 2) hipLaunchKernelGGL((KERNEL<2>), __VA_ARGS__);      \
        else if ((N) <= 4) hipLaunchKernelGGL((KERNEL<4>), __VA_ARGS__);      \
        else if ((N) <= 8) hipLaunchKernelGGL((KERNEL<8>), __VA_ARGS__);      \
        else hipLaunchKernelGGL((KERNEL<16>), __VA_ARGS__);                   \
    } while (0)

extern "C" int tdr_kvproj_tile_rows(void) { return PROJ_R; }

extern "C" int tdr_kvproj_fwd(const void* table, int nseg, int64_t ntiles, const float* kv, int N, int K, float* out, int64_t ld,
                              void* stream) {
    TDR_REQUIRE(table && kv && out && nseg > 0 && ntiles > 0, "tdr_kvproj_fwd: null pointer / empty table");
    TDR_REQUIRE(N >= 1 && N <= 16 && K > 0 && K % 256 == 0, "tdr_kvproj_fwd: need 1 <= N <= 16 and K %% 256 == 0 (N=%d K=%d)", N, K);
    hipStream_t st = (hipStream_t)stream;
    KVP_DISPATCH(kvproj_fwd_kernel, N, dim3(tdr_cdiv(ntiles, 4)), dim3(256), 0, st, (const long*)table, nseg, (long)ntiles, kv, N, K,
                 out, (long)ld);
    TDR_LAUNCH_CHECK("kvproj_fwd");
    return TDR_OK;
}

extern "C" int tdr_kvproj_wgrad(const void* table, const void* gtable, int nseg, int64_t ntiles, const float* kv, const float* dk,
                                int64_t ld, int N, int K, void* stream) {
    TDR_REQUIRE(table && gtable && kv && dk && nseg > 0 && ntiles > 0, "tdr_kvproj_wgrad: null pointer / empty table");
    TDR_REQUIRE(N >= 1 && N <= 16 && K > 0 && K % 1024 == 0, "tdr_kvproj_wgrad: need 1 <= N <= 16 and K %% 1024 == 0");
    hipStream_t st = (hipStream_t)stream;
    KVP_DISPATCH(kvproj_wgrad_kernel, N, dim3((unsigned)ntiles), dim3(256), 0, st, (const long*)table, (const long*)gtable, nseg, kv,
                 dk, (long)ld, N, K);
    TDR_LAUNCH_CHECK("kvproj_wgrad");
    return TDR_OK;
}

extern "C" int tdr_kvproj_dkv_parts(int64_t ntiles) {
    const long want = 192;                      // first-stage row groups: with K / 1024 = 10 column blocks ~1900 workgroups
    return (int)(ntiles < want ? ntiles : want);
}

extern "C" int64_t tdr_kvproj_dkv_ws_floats(int64_t ntiles, int N, int K) {
    return (int64_t)tdr_kvproj_dkv_parts(ntiles) * N * K;
}

extern "C" int tdr_kvproj_dkv(const void* table, int nseg, int64_t ntiles, const float* dk, int64_t ld, int N, int K, float* dkv,
                              float* ws, void* stream) {
    TDR_REQUIRE(table && dk && dkv && ws && nseg > 0 && ntiles > 0, "tdr_kvproj_dkv: null pointer / empty table");
    TDR_REQUIRE(N >= 1 && N <= 16 && K > 0 && K % 4 == 0, "tdr_kvproj_dkv: need 1 <= N <= 16 and K %% 4 == 0");
    hipStream_t st = (hipStream_t)stream;
    const int S = tdr_kvproj_dkv_parts(ntiles);
    const int tpb = tdr_cdiv(ntiles, S);
    const int Sused = tdr_cdiv(ntiles, tpb);
    KVP_DISPATCH(kvproj_dkv_part_kernel, N, dim3(tdr_cdiv(K, 1024), Sused), dim3(256), 0, st, (const long*)table, nseg, (long)ntiles,
                 tpb, dk, (long)ld, N, K, ws);
    TDR_LAUNCH_CHECK("kvproj_dkv_part");
    const long len = (long)N * K;
    hipLaunchKernelGGL(kvproj_dkv_finish_kernel, dim3(tdr_cdiv(len, 256)), dim3(256), 0, st, ws, Sused, len, dkv);
    TDR_LAUNCH_CHECK("kvproj_dkv_finish");
    return TDR_OK;
}

extern "C" int tdr_modln_fwd(const float* x, const float* a, const float* b, int64_t ab_ns, const float* w, const float* lb, float eps,
                             int N, int C, int HW, float* y, float* mu, float* rstd, void* stream) {
    TDR_REQUIRE(x && a && b && w && lb && y && mu && rstd, "tdr_modln_fwd: null pointer");
    TDR_REQUIRE(N > 0 && C > 0 && HW > 0, "tdr_modln_fwd: bad shape");
    hipLaunchKernelGGL(modln_fwd_kernel, dim3(tdr_cdiv(HW, 64), N), dim3(1024), 0, (hipStream_t)stream, x, a, b, (long)ab_ns, w, lb, eps,
                       C, HW, y, mu, rstd);
    TDR_LAUNCH_CHECK("modln_fwd");
    return TDR_OK;
}

extern "C" int tdr_nc_affine(const float* x, const float* a, const float* b, int64_t ab_ns, int N, int C, int HW, float* y, void* stream) {
    TDR_REQUIRE(x && a && b && y && N > 0 && C > 0 && HW > 0, "tdr_nc_affine: bad arguments");
    const long total = (long)N * C * HW;
    hipLaunchKernelGGL(nc_affine_kernel, dim3(tdr_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, a, b, (long)ab_ns, C, HW,
                       total, y);
    TDR_LAUNCH_CHECK("nc_affine");
    return TDR_OK;
}

extern "C" int tdr_nc_affine_bwd(const float* dm, const float* x, const float* a, int64_t ab_ns, const float* add, int N, int C, int HW,
                                 float* dx, float* da, float* db, int64_t d_ns, void* stream) {
    TDR_REQUIRE(dm && x && a && dx && da && db && N > 0 && C > 0 && HW > 0, "tdr_nc_affine_bwd: bad arguments");
    hipLaunchKernelGGL(nc_affine_bwd_kernel, dim3(N * C), dim3(256), 0, (hipStream_t)stream, dm, x, a, (long)ab_ns, add, C, HW, dx, da,
                       db, (long)d_ns);
    TDR_LAUNCH_CHECK("nc_affine_bwd");
    return TDR_OK;
}

extern "C" int tdr_modgate_fwd(const float* t, const float* a, const float* b, int64_t ab_ns, int N, int c, int HW, float* g,
                               float* pooled, void* stream) {
    TDR_REQUIRE(t && a && b && g && N > 0 && c > 0 && HW > 0, "tdr_modgate_fwd: bad arguments");
    hipLaunchKernelGGL(modgate_fwd_kernel, dim3(N * c), dim3(256), 0, (hipStream_t)stream, t, a, b, (long)ab_ns, c, HW, g, pooled);
    TDR_LAUNCH_CHECK("modgate_fwd");
    return TDR_OK;
}

extern "C" int tdr_modgate_bwd(const float* dg, const float* dgb, float dgb_mul, const float* t, const float* a, const float* b,
                               int64_t ab_ns, int N, int c, int HW, float* dt, float* da, float* db, int64_t d_ns, void* stream) {
    TDR_REQUIRE(dg && t && a && b && dt && da && db && N > 0 && c > 0 && HW > 0, "tdr_modgate_bwd: bad arguments");
    hipLaunchKernelGGL(modgate_bwd_kernel, dim3(N * c), dim3(256), 0, (hipStream_t)stream, dg, dgb, dgb_mul, t, a, b, (long)ab_ns, c, HW,
                       dt, da, db, (long)d_ns);
    TDR_LAUNCH_CHECK("modgate_bwd");
    return TDR_OK;
}
