// FFTLoss: the frequency-domain L1 criterion w * mean | stack(Re, Im)(fft2(pred) - fft2(target)) | (two-sided; the rfft2 variant with
// onesided), value and gradient, for P = N C independent planes [H][W].  The definition is in include/tdr.h (tdr_freq_loss).
//
//   table   : tw_W[t] = exp(-2 pi i t / W), tw_H likewise, computed in double and rounded once, and the two digit-reversal tables (the
//             place of frequency kx along W, the frequency at each place along H): W + H entries each, one small launch.
//   rows    : d = pred - target while loading; TWO real rows ride one complex FFT along W (z = row_a + i row_b) in LDS, in place
//             (tdr_fft_core.h: forward decimation in frequency, digit-reversed out); A[k], B[k] for k <= W/2 are split from Z[k] and
//             Z[W - k] at their digit-reversed places and go to the workspace [P][H][W/2+1] complex in NATURAL kx order.
//   columns : a workgroup of 1024 threads owns TC adjacent kx of one plane (TC = 16, 128 B per row segment; 8 for H = 1024), all H rows,
//             in LDS as [H][TC] complex without padding, the H twiddles behind it: a wave takes 8 neighbouring butterflies of 8
//             neighbouring columns (or 4 of 16), so its 64 8-byte accesses are whole rows of the tile.  Forward FFT along H in place; at the digit-reversed places the bin is decided
//             (self-conjugate bins lose their imaginary part), optionally written to `spec`, summed as c (|Re| + |Im|) and replaced by
//             Gh = m (sgn Re + i sgn Im); the inverse stages over the same radices in reverse bring the natural row order back with no
//             reordering pass, and the tile returns to the workspace.  The forward spectrum never reaches HBM unless `spec` asks.
//   rows^-1 : Z[k] = A[k] + i B[k], Z[W - k] = conj A[k] + i conj B[k] (the imaginary parts of kx = 0, W/2 ignored, as irfft does), inverse
//             FFT, row_a = Re z, row_b = Im z, times scale * w / count, stored or added.
//   finish  : one workgroup folds the per-workgroup partials (doubles) in a fixed order.
// No atomics, no host synchronisation; the same call gives the same bits.
#include <atomic>

#include "tdr_common.h"
#include "tdr_fft_core.h"
#include "../../include/tdr.h"

namespace {

using tdr_fft::Plan;

constexpr int NT = 256;
constexpr int NTC = 1024;                // the column pass: 16 waves hide the LDS latency of the stages between barriers
constexpr int ROW_ELEMS = 1024;          // complex elements of a row workgroup's LDS: max(1, 1024 / W) row pairs
constexpr int ROW_LDS = ROW_ELEMS + ROW_ELEMS / 32;      // with the spare element after every 32 (tdr_fft::pad32)

// rev[kx] for kx < W: the place of frequency kx after the forward stages along W; rev[W + pos]: the frequency at place pos along H
__global__ __launch_bounds__(NT) void freq_table_kernel(float2* __restrict__ tw, int* __restrict__ rev, Plan pw, Plan ph) {
    const int i = blockIdx.x * NT + threadIdx.x, W = pw.L, H = ph.L;
    if (i >= W + H) return;
    const int L = i < W ? W : H, t = i < W ? i : i - W;
    double s, c;
    sincospi(-2.0 * (double)t / (double)L, &s, &c);
    tw[i] = make_float2((float)c, (float)s);
    rev[i] = i < W ? tdr_fft::fft_pos_of(pw, t) : tdr_fft::fft_freq_at(ph, t);
}

struct RowArgs {
    const float* pred; const float* target;        // forward
    float2* ws;                                    // [P*H][WP]
    const float2* tw;                              // [W]
    const int* rev;                                // [W]: the place of each kx
    float* dpred;                                  // inverse
    const TdrStepGuard* guard;
    float base, gscale;
    int accumulate;
    int W, WP, rpb;                                // rpb: row pairs per workgroup
    int64_t npairs;                                // P * H / 2
    Plan plan;
};

__device__ __forceinline__ float scaled_term(float coef, float x, float old, int accumulate) {
#pragma clang fp contract(off)
    const float t = coef * x;
    return accumulate ? old + t : t;
}

__global__ __launch_bounds__(NT) void freq_rows_fwd_kernel(RowArgs p) {
    __shared__ float2 buf[ROW_LDS];
    __shared__ float2 tw[tdr_fft::MAX_LEN];
    __shared__ int rev[tdr_fft::MAX_LEN];
    const int tid = threadIdx.x, W = p.W, PL = tdr_fft::pad32(p.W);      // PL: the pitch of a padded line (W elements and their spares)
    const int64_t g0 = (int64_t)blockIdx.x * p.rpb;
    const int npl = (int)min((int64_t)p.rpb, p.npairs - g0);          // pairs of this workgroup (>= 1 by the grid)
    for (int i = tid; i < W; i += NT) { tw[i] = p.tw[i]; rev[i] = p.rev[i]; }
    for (int i = tid; i < npl * W; i += NT) {
        const int l = i / W, x = i - l * W;
        const int64_t o = (g0 + l) * 2 * W + x;
        buf[l * PL + tdr_fft::pad32(x)] = make_float2(p.pred[o] - p.target[o], p.pred[o + W] - p.target[o + W]);
    }
    __syncthreads();
    tdr_fft::forward<false>(p.plan, buf, npl, PL, 1, tw, tid, NT);
    for (int i = tid; i < npl * p.WP; i += NT) {
        const int l = i / p.WP, k = i - l * p.WP;
        const float2 zk = buf[l * PL + tdr_fft::pad32(rev[k])];
        const float2 zn = buf[l * PL + tdr_fft::pad32(rev[k ? W - k : 0])];
        float2 a, b;
        tdr_fft::split_pair(zk, zn, a, b);
        float2* o = p.ws + (g0 + l) * 2 * p.WP + k;
        o[0] = a;
        o[p.WP] = b;
    }
}

__global__ __launch_bounds__(NT) void freq_rows_inv_kernel(RowArgs p) {
    __shared__ float2 buf[ROW_LDS];
    __shared__ float2 tw[tdr_fft::MAX_LEN];
    __shared__ int rev[tdr_fft::MAX_LEN];
    const int tid = threadIdx.x, W = p.W, PL = tdr_fft::pad32(p.W);      // PL: the pitch of a padded line (W elements and their spares)
    const int64_t g0 = (int64_t)blockIdx.x * p.rpb;
    const int npl = (int)min((int64_t)p.rpb, p.npairs - g0);
    float gscale = p.gscale;
    if (p.guard) gscale *= p.guard->scale;             // powers of two: exact
    const float coef = p.base * gscale;
    for (int i = tid; i < W; i += NT) { tw[i] = p.tw[i]; rev[i] = p.rev[i]; }
    for (int i = tid; i < npl * p.WP; i += NT) {
        const int l = i / p.WP, k = i - l * p.WP;
        const float2* o = p.ws + (g0 + l) * 2 * p.WP + k;
        float2 a = o[0], b = o[p.WP];
        const bool edge = k == 0 || 2 * k == W;
        if (edge) { a.y = 0.f; b.y = 0.f; }
        float2 zk, zn;
        tdr_fft::merge_pair(a, b, zk, zn);
        buf[l * PL + tdr_fft::pad32(rev[k])] = zk;
        if (!edge) buf[l * PL + tdr_fft::pad32(rev[W - k])] = zn;
    }
    __syncthreads();
    tdr_fft::inverse<false>(p.plan, buf, npl, PL, 1, tw, tid, NT);
    for (int i = tid; i < npl * W; i += NT) {
        const int l = i / W, x = i - l * W;
        const int64_t o = (g0 + l) * 2 * W + x;
        const float2 z = buf[l * PL + tdr_fft::pad32(x)];
        p.dpred[o] = scaled_term(coef, z.x, p.accumulate ? p.dpred[o] : 0.f, p.accumulate);
        p.dpred[o + W] = scaled_term(coef, z.y, p.accumulate ? p.dpred[o + W] : 0.f, p.accumulate);
    }
}

struct ColArgs {
    float2* ws;                  // [P][H][WP]
    const float2* tw;            // [H]
    const int* rev;              // [H]: the frequency at each place
    float2* spec;                // [P][H][WP] or null
    double* partial;             // [P][tiles]
    int H, W, WP, tc;            // tc: columns of a tile, 8 or 16
    int onesided, inverse;
    Plan plan;
};

__device__ __forceinline__ float sgn0(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

__global__ __launch_bounds__(NTC) void freq_cols_kernel(ColArgs p) {
    constexpr int NT = NTC;
    extern __shared__ __attribute__((aligned(16))) float2 tile[];          // [H][tc], then the H twiddles
    const int tid = threadIdx.x, H = p.H, tc = p.tc, WP = p.WP;
    const int kx0 = blockIdx.x * tc;
    const int64_t plane = (int64_t)blockIdx.y * H * WP;
    float2* src = p.ws + plane;
    const int total = H * tc, csh = __builtin_ctz(tc);
    float2* tw = tile + total;
    for (int i = tid; i < H; i += NT) tw[i] = p.tw[i];
    for (int i = tid; i < total; i += NT) {
        const int y = i >> csh, c = i & (tc - 1);
        tile[i] = kx0 + c < WP ? src[(int64_t)y * WP + kx0 + c] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    tdr_fft::forward<true>(p.plan, tile, tc, 1, tc, tw, tid, NT);
    double acc = 0.0;                                      // <= 64 bins per thread; double keeps the value at the error of the bins
    for (int i = tid; i < total; i += NT) {
        const int pos = i >> csh, c = i & (tc - 1), kx = kx0 + c;
        if (kx >= WP) continue;                            // the inverse of a zero column stays unused
        const int ky = p.rev[pos];
        const bool xedge = kx == 0 || 2 * kx == p.W;
        float2 d = tile[i];
        if (xedge && (ky == 0 || 2 * ky == H)) d.y = 0.f;
        if (p.spec) p.spec[plane + (int64_t)ky * WP + kx] = d;
        const float cw = (p.onesided || xedge) ? 1.f : 2.f;
        acc += (double)(cw * (fabsf(d.x) + fabsf(d.y)));
        const float m = (p.onesided && !xedge) ? 0.5f : 1.f;
        tile[i] = make_float2(m * sgn0(d.x), m * sgn0(d.y));
    }
    __syncthreads();
    if (p.inverse) {
        tdr_fft::inverse<true>(p.plan, tile, tc, 1, tc, tw, tid, NT);
        for (int i = tid; i < total; i += NT) {
            const int y = i >> csh, c = i & (tc - 1);
            if (kx0 + c < WP) src[(int64_t)y * WP + kx0 + c] = tile[i];
        }
        __syncthreads();                                   // the tile is reused by the fold below
    }
    double* red = reinterpret_cast<double*>(tile);         // 16 doubles; the smallest tile (H = 4, 16 columns) has 512 bytes
    double v = acc;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_down(v, o, 64);
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int i = 0; i < NT / 64; ++i) s += red[i];
        p.partial[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(NT) void freq_finish_kernel(const double* __restrict__ partial, int64_t n, double w, double count,
                                                        float* __restrict__ loss) {
    __shared__ double red[NT];
    double acc = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += NT) acc += partial[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = NT / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(w * red[0] / count);
}

struct FreqWs { int64_t tw, rev, partial, spec, total; int tc, tiles; };

FreqWs freq_ws(int N, int C, int H, int W) {
    const int64_t P = (int64_t)N * C, WP = W / 2 + 1;
    FreqWs o;
    o.tc = H > 512 ? 8 : 16;
    o.tiles = tdr_cdiv(WP, o.tc);
    o.tw = 0;
    o.rev = (int64_t)(W + H) * 8;
    o.partial = (o.rev + (int64_t)(W + H) * 4 + 15) & ~(int64_t)15;
    o.spec = (o.partial + P * o.tiles * 8 + 15) & ~(int64_t)15;
    o.total = o.spec + P * H * WP * 8;
    return o;
}

constexpr int MAX_DEVICES = 64;
constexpr int MAX_PLANES = 65535;        // the plane index is blockIdx.y of the column pass

}  // namespace

extern "C" int tdr_freq_loss_takes(int H, int W) { return tdr_fft::admissible(H) && tdr_fft::admissible(W) ? 1 : 0; }

extern "C" int64_t tdr_freq_loss_ws_bytes(int N, int C, int H, int W) {
    if (N < 1 || C < 1 || (int64_t)N * C > MAX_PLANES || !tdr_freq_loss_takes(H, W)) return 0;
    return freq_ws(N, C, H, W).total;
}

extern "C" int tdr_freq_loss(const float* pred, const float* target, int N, int C, int H, int W, int onesided, float loss_weight,
                             float grad_scale, const TdrStepGuard* guard, int accumulate, float* loss, float* dpred, float* spec, void* ws,
                             void* stream) {
    TDR_REQUIRE(pred && target && loss && ws, "tdr_freq_loss: null pointer (pred, target, loss, ws)");
    TDR_REQUIRE(tdr_freq_loss_takes(H, W),
                "tdr_freq_loss: %d x %d: H and W must each be m * 2^a with m in {1, 3, 5}, a >= 2, 4 <= length <= 1024", H, W);
    TDR_REQUIRE(N >= 1 && C >= 1 && (int64_t)N * C <= MAX_PLANES, "tdr_freq_loss: N %d, C %d: N, C >= 1 and N * C <= %d planes", N, C,
                MAX_PLANES);
    const FreqWs L = freq_ws(N, C, H, W);
    const int64_t P = (int64_t)N * C;
    const int WP = W / 2 + 1;
    char* base = static_cast<char*>(ws);
    hipStream_t st = (hipStream_t)stream;
    float2* tw = reinterpret_cast<float2*>(base + L.tw);
    double* partial = reinterpret_cast<double*>(base + L.partial);
    const double count = 2.0 * (double)P * H * (onesided ? (double)WP : (double)W);

    // the column pass needs up to 72 KiB of dynamic LDS: the limit is raised once per device (setting it twice from two threads is harmless)
    static std::atomic<bool> attr_set[MAX_DEVICES];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAX_DEVICES) {
        tdr_set_error("tdr_freq_loss: no current device below %d", MAX_DEVICES);
        return TDR_ERR_HIP;
    }
    if (!attr_set[dev].load()) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(freq_cols_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 72 * 1024) !=
            hipSuccess) {
            (void)hipGetLastError();
            tdr_set_error("tdr_freq_loss: cannot raise the dynamic LDS limit of the column pass to 72 KiB on device %d", dev);
            return TDR_ERR_HIP;
        }
        attr_set[dev].store(true);
    }
    int* rev = reinterpret_cast<int*>(base + L.rev);
    const Plan pw = tdr_fft::make_plan(W), ph = tdr_fft::make_plan(H, L.tc == 8);      // (8-column tiles: see make_plan)
    hipLaunchKernelGGL(freq_table_kernel, dim3(tdr_cdiv(W + H, NT)), dim3(NT), 0, st, tw, rev, pw, ph);
    TDR_LAUNCH_CHECK("freq_table_kernel");

    RowArgs r;
    r.pred = pred; r.target = target;
    r.ws = reinterpret_cast<float2*>(base + L.spec);
    r.tw = tw;
    r.rev = rev;
    r.dpred = dpred;
    r.guard = guard;
    r.base = (float)((double)loss_weight / count);
    r.gscale = grad_scale;
    r.accumulate = accumulate ? 1 : 0;
    r.W = W; r.WP = WP;
    r.rpb = ROW_ELEMS / W;
    r.npairs = P * (H / 2);
    r.plan = pw;
    const dim3 rgrid((unsigned)((r.npairs + r.rpb - 1) / r.rpb));
    hipLaunchKernelGGL(freq_rows_fwd_kernel, rgrid, dim3(NT), 0, st, r);
    TDR_LAUNCH_CHECK("freq_rows_fwd_kernel");

    ColArgs c;
    c.ws = r.ws;
    c.tw = tw + W;
    c.rev = rev + W;
    c.spec = reinterpret_cast<float2*>(spec);
    c.partial = partial;
    c.H = H; c.W = W; c.WP = WP; c.tc = L.tc;
    c.onesided = onesided ? 1 : 0;
    c.inverse = dpred ? 1 : 0;
    c.plan = ph;
    const size_t lds = ((size_t)H * L.tc + H) * sizeof(float2);            // at most 64 + 8 KiB: above the 64 KiB a kernel gets unasked
    hipLaunchKernelGGL(freq_cols_kernel, dim3(L.tiles, (unsigned)P), dim3(NTC), lds, st, c);
    TDR_LAUNCH_CHECK("freq_cols_kernel");

    hipLaunchKernelGGL(freq_finish_kernel, dim3(1), dim3(NT), 0, st, partial, P * L.tiles, (double)loss_weight, count, loss);
    TDR_LAUNCH_CHECK("freq_finish_kernel");
    if (!dpred) return TDR_OK;

    hipLaunchKernelGGL(freq_rows_inv_kernel, rgrid, dim3(NT), 0, st, r);
    TDR_LAUNCH_CHECK("freq_rows_inv_kernel");
    return TDR_OK;
}
