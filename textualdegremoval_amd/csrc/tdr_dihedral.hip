// Geometric self-ensemble (inference.InferenceSession.run_ensemble): the two passes around the forwards when a network runs on the flips
// and transposes of an image and the eight answers are averaged (`test_x8` of KAIR, `self_ensemble` of BasicSR).
//   tdr_dihedral_gather : the selected transforms of the images, all of one class (straight: ops 0-3, shape kept; transposed: ops 4-7,
//                         (H, W) -> (W, H)):  float32 [N][C][H][W] or uint8 [N][H][W][C]  ->  float32 [K][N][C][Ho][Wo]
//   tdr_dihedral_mean   : every member transformed back, added in ascending op order, divided by their number:
//                         float32 [Ks][N][C][H][W] + float32 [Kt][N][C][W][H]  ->  float32 [N][C][H][W] or uint8 [N][H][W][C]
// Op code: bit 0 the horizontal flip (x -> W-1-x), bit 1 the vertical flip (y -> H-1-y), bit 2 the transpose, applied after the flips.
// Streaming kernels in the style of tdr_tile.hip, one thread per 4 pixels of a row: a float4 where base and pitch are 16-byte aligned and
// the 4 pixels lie inside the row, pixel by pixel otherwise; interleaved bytes as C 32-bit words where the 4-pixel group starts on a word.
// A flipped row is still one contiguous segment per wave, read from its far end: the 4 pixels of a thread arrive as one float4 and are
// reversed in registers, so the straight ops need no LDS.
// A transpose goes through a 32 x 32 LDS tile of row pitch 33 floats: 256 threads read 32 rows of 8 float4 and write it as [r][4q + i],
// bank (r + 4q + i) % 32 -- the 32 lanes of a half hold 4 rows x 8 float4, 32 different banks; they then read it as [4q + i][r], bank
// (4q + i + r) % 32, again 32 different banks, and store rows of the transposed plane: both global sides stay row-contiguous.
// Bytes go through the 256-entry float32(u) / 255.0f table of tdr_img_u8_to_planes (the same division, computed on the host); the way
// back is tdr_planes_to_img_u8's: fminf / fmaxf, one float32 product with 255.0f, rintf -- on the very float the float output holds.
// The sum is fp32 without contraction and starts from the first member itself; one IEEE division by float32(n) ends it.
// All sizes and masks arrive by value: no device tables, no atomics; nothing outside the tensors the sizes describe is read or written.
#include "tdr_common.h"
#include "../../include/tdr.h"

#pragma clang fp contract(off)

namespace {

constexpr int TS = 32;                 // the LDS tile: TS x TS floats ...
constexpr int PITCH = TS + 1;          // ... of an odd row pitch

struct U8Table { float v[256]; };

// the k-th selected op of a mask (bit `op` set = op selected), ascending
__device__ __forceinline__ int nth_op(int mask, int k) {
    for (int op = 0; op < 8; ++op)
        if ((mask >> op) & 1) {
            if (k == 0) return op;
            --k;
        }
    return 0;
}

__device__ __forceinline__ void load4(const float* __restrict__ s, bool vec, bool reversed, int left, float v[4]) {
    // 4 values of a row from s[0 .. 3] (reversed: v[i] = s[3 - i]); `left` of them exist: the first of v, wherever they lie in s
    if (vec && left >= 4) {
        const float4 f = *reinterpret_cast<const float4*>(s);
        if (reversed) { v[0] = f.w; v[1] = f.z; v[2] = f.y; v[3] = f.x; }
        else { v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w; }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < left) v[i] = reversed ? s[3 - i] : s[i];
    }
}

__device__ __forceinline__ void store4(float* __restrict__ d, bool vec, bool reversed, int left, const float v[4]) {
    // the mirror of load4: d[i] = v[i] (reversed: d[3 - i] = v[i]) for the first `left` of v
    if (vec && left >= 4) {
        *reinterpret_cast<float4*>(d) = reversed ? make_float4(v[3], v[2], v[1], v[0]) : make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < left) d[reversed ? 3 - i : i] = v[i];
    }
}

// ---- gather, straight class: out[k][p][y][x] = src[p][fy(y)][fx(x)]
__global__ __launch_bounds__(256) void dihedral_gather_straight_f32_kernel(const float* __restrict__ src, long planes, int H, int W, int mask,
                                                                           int K, float* __restrict__ out, int vec_src, int vec_dst) {
    const int groups = (W + 3) >> 2;
    const long total = (long)K * planes * H * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % groups);
    long row = t / groups;
    const int y = (int)(row % H);
    row /= H;
    const long p = row % planes;
    const int k = (int)(row / planes), x = g << 2, op = nth_op(mask, k);
    const int left = min(4, W - x);
    const bool hf = op & 1;
    const float* srow = src + (p * H + ((op & 2) ? H - 1 - y : y)) * W;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    load4(hf ? srow + (W - 4 - x) : srow + x, vec_src, hf, left, v);      // (reversed: s[3 - i] = srow[W - 1 - x - i], i < left: inside the row)
    store4(out + (((long)k * planes + p) * H + y) * W + x, vec_dst, false, left, v);
}

template <int C>
__global__ __launch_bounds__(256) void dihedral_gather_straight_u8_kernel(const uint8_t* __restrict__ img, int N, int H, int W, int swap, int mask,
                                                                          int K, float* __restrict__ out, int word_src, int vec_dst, U8Table tab) {
    __shared__ float lut[256];
    lut[threadIdx.x] = tab.v[threadIdx.x];
    __syncthreads();
    const int groups = (W + 3) >> 2;
    const long total = (long)K * N * H * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % groups);
    long row = t / groups;
    const int y = (int)(row % H);
    row /= H;
    const int n = (int)(row % N), k = (int)(row / N), x = g << 2, op = nth_op(mask, k);
    const bool hf = op & 1;
    const uint8_t* srow = img + ((long)n * H + ((op & 2) ? H - 1 - y : y)) * W * C;
    float v[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = 0.f;
    if (word_src && x + 3 < W) {                                       // 4 whole pixels, 4 * C bytes from a word boundary
        const uint32_t* s4 = reinterpret_cast<const uint32_t*>(srow + (long)(hf ? W - 4 - x : x) * C);
        uint32_t w[C];
#pragma unroll
        for (int j = 0; j < C; ++j) w[j] = s4[j];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int q = i * C + c;
                const float f = lut[(w[q >> 2] >> ((q & 3) * 8)) & 0xff];
                if (hf) v[c][3 - i] = f;
                else v[c][i] = f;
            }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < W) {
                const uint8_t* s = srow + (long)(hf ? W - 1 - x - i : x + i) * C;
#pragma unroll
                for (int c = 0; c < C; ++c) v[c][i] = lut[s[c]];
            }
    }
    const int left = min(4, W - x);
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int cr = C == 3 ? 2 - c : c;                             // swapped: plane c holds byte channel 2 - c
        store4(out + ((((long)k * N + n) * C + c) * H + y) * W + x, vec_dst, false, left, (C == 3 && swap) ? v[cr] : v[c]);
    }
}

// ---- gather, transposed class: out[k][p][i][j] = src[p][fy(j)][fx(i)], a [W][H] plane.  One workgroup per 32 x 32 tile of a source plane.
// the tile's store: thread (r, q) holds source column x0 + r = one output row, source rows y0 + q ... y0 + q + 3 = 4 output columns
__device__ __forceinline__ void store_transposed(const float* __restrict__ lds, float* __restrict__ plane, int op, int H, int W, int y0, int x0,
                                                 int r, int q, int vec_dst) {
    const int x = x0 + r, yq = y0 + q;
    if (x >= W || yq >= H) return;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = lds[(q + i) * PITCH + r];
    float* d = plane + (long)((op & 1) ? W - 1 - x : x) * H;
    const bool vf = op & 2;
    store4(vf ? d + (H - 4 - yq) : d + yq, vec_dst, vf, min(4, H - yq), v);   // (reversed: d[3 - i] = row[H - 1 - yq - i], i < left)
}

__global__ __launch_bounds__(256) void dihedral_gather_transposed_f32_kernel(const float* __restrict__ src, long planes, int H, int W, int mask,
                                                                             float* __restrict__ out, int vec_src, int vec_dst) {
    __shared__ float lds[TS * PITCH];
    const int tiles_x = (W + TS - 1) / TS, tiles_y = (H + TS - 1) / TS;
    long b = blockIdx.x;
    const int x0 = (int)(b % tiles_x) * TS;
    b /= tiles_x;
    const int y0 = (int)(b % tiles_y) * TS;
    b /= tiles_y;
    const long p = b % planes;
    const int k = (int)(b / planes), op = nth_op(mask, k);
    const int r = threadIdx.x >> 3, q = (threadIdx.x & 7) << 2;
    if (y0 + r < H && x0 + q < W) {
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        load4(src + (p * H + y0 + r) * W + x0 + q, vec_src, false, min(4, W - x0 - q), v);
#pragma unroll
        for (int i = 0; i < 4; ++i) lds[r * PITCH + q + i] = v[i];
    }
    __syncthreads();
    store_transposed(lds, out + ((long)k * planes + p) * H * W, op, H, W, y0, x0, r, q, vec_dst);
}

template <int C>
__global__ __launch_bounds__(256) void dihedral_gather_transposed_u8_kernel(const uint8_t* __restrict__ img, int N, int H, int W, int swap, int mask,
                                                                            float* __restrict__ out, int word_src, int vec_dst, U8Table tab) {
    __shared__ float lut[256];
    __shared__ float lds[C][TS * PITCH];
    lut[threadIdx.x] = tab.v[threadIdx.x];
    __syncthreads();
    const int tiles_x = (W + TS - 1) / TS, tiles_y = (H + TS - 1) / TS;
    long b = blockIdx.x;
    const int x0 = (int)(b % tiles_x) * TS;
    b /= tiles_x;
    const int y0 = (int)(b % tiles_y) * TS;
    b /= tiles_y;
    const int n = (int)(b % N), k = (int)(b / N), op = nth_op(mask, k);
    const int r = threadIdx.x >> 3, q = (threadIdx.x & 7) << 2;
    if (y0 + r < H && x0 + q < W) {
        const uint8_t* s = img + (((long)n * H + y0 + r) * W + x0 + q) * C;
        if (word_src && x0 + q + 3 < W) {                              // 4 whole pixels, 4 * C bytes from a word boundary
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
            uint32_t w[C];
#pragma unroll
            for (int j = 0; j < C; ++j) w[j] = s4[j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int e = i * C + c;
                    lds[c][r * PITCH + q + i] = lut[(w[e >> 2] >> ((e & 3) * 8)) & 0xff];
                }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + q + i < W) {
#pragma unroll
                    for (int c = 0; c < C; ++c) lds[c][r * PITCH + q + i] = lut[s[i * C + c]];
                }
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int cs = (C == 3 && swap) ? 2 - c : c;                   // swapped: plane c holds byte channel 2 - c
        store_transposed(lds[cs], out + (((long)k * N + n) * C + c) * H * W, op, H, W, y0, x0, r, q, vec_dst);
    }
}

// ---- mean.  One workgroup per 32 x 32 tile of the output: thread (r, q) owns the 4 pixels (y0 + r, x0 + q ... x0 + q + 3).  CU8 = 0: float
// output, one plane per workgroup; CU8 = C: byte output, the C planes of an image one after the other, so that a thread ends up with the
// C bytes of its 4 pixels.  The transposed members of a plane ([W][H]) are staged through LDS, one tile each, as the gather's stores in
// reverse: thread (r, q) reads row fx(x0 + r), columns fy(y0 + q ...) and writes [q + i][r]; the sum then reads [r][q + i].
__device__ __forceinline__ uint32_t to_u8(float x) {
    x = fminf(fmaxf(x, 0.f), 1.f);
    return (uint32_t)rintf(x * 255.0f);
}

template <int CU8>
__global__ __launch_bounds__(256) void dihedral_mean_kernel(const float* __restrict__ straight, int mask_s, const float* __restrict__ transposed,
                                                            int mask_t, int N, int C, int H, int W, float* __restrict__ out_f32,
                                                            uint8_t* __restrict__ out_u8, int swap, float count, int vec_s, int vec_t, int vec_o) {
    constexpr int NC = CU8 ? CU8 : 1;
    __shared__ float lds[4][TS * PITCH];
    const int tiles_x = (W + TS - 1) / TS, tiles_y = (H + TS - 1) / TS;
    long b = blockIdx.x;
    const int x0 = (int)(b % tiles_x) * TS;
    b /= tiles_x;
    const int y0 = (int)(b % tiles_y) * TS;
    b /= tiles_y;                                                      // the plane n * C + c (float output) / the image n (byte output)
    const long planes = (long)N * C;
    const int r = threadIdx.x >> 3, q = (threadIdx.x & 7) << 2;
    const int y = y0 + r, x = x0 + q;
    const bool mine = y < H && x < W;
    const int left = min(4, W - x);
    float res[NC][4];
#pragma unroll
    for (int ci = 0; ci < NC; ++ci) {
        const long p = CU8 ? b * C + ci : b;
        if (mask_t) {
            if (ci) __syncthreads();                                   // the previous plane's tiles have been read
            const int ox = x0 + r, yq = y0 + q;
            if (ox < W && yq < H) {
                int m = 0;
                for (int op = 4; op < 8; ++op) {
                    if (!((mask_t >> op) & 1)) continue;
                    const float* s = transposed + (((long)m * planes + p) * W + ((op & 1) ? W - 1 - ox : ox)) * H;
                    const bool vf = op & 2;
                    float v[4] = {0.f, 0.f, 0.f, 0.f};
                    load4(vf ? s + (H - 4 - yq) : s + yq, vec_t, vf, min(4, H - yq), v);
#pragma unroll
                    for (int i = 0; i < 4; ++i) lds[m][(q + i) * PITCH + r] = v[i];
                    ++m;
                }
            }
            __syncthreads();
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (mine) {
            bool first = true;
            int m = 0;
            for (int op = 0; op < 4; ++op) {
                if (!((mask_s >> op) & 1)) continue;
                const float* s = straight + (((long)m * planes + p) * H + ((op & 2) ? H - 1 - y : y)) * W;
                const bool hf = op & 1;
                float v[4] = {0.f, 0.f, 0.f, 0.f};
                load4(hf ? s + (W - 4 - x) : s + x, vec_s, hf, left, v);
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = first ? v[i] : acc[i] + v[i];
                first = false;
                ++m;
            }
            m = 0;
            for (int op = 4; op < 8; ++op) {
                if (!((mask_t >> op) & 1)) continue;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = lds[m][r * PITCH + q + i];
                    acc[i] = first ? v : acc[i] + v;
                }
                first = false;
                ++m;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) res[ci][i] = acc[i] / count;
    }
    if (!mine) return;
    if (CU8 == 0) {
        store4(out_f32 + (b * H + y) * W + x, vec_o, false, left, res[0]);
        return;
    }
    uint32_t u[NC][4];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const int cs = (NC == 3 && swap) ? 2 - c : c;                  // swapped: byte channel c holds plane 2 - c
#pragma unroll
        for (int i = 0; i < 4; ++i) u[c][i] = to_u8(res[cs][i]);
    }
    uint8_t* dst = out_u8 + ((b * H + y) * W + x) * NC;
    if (vec_o && left >= 4) {                                          // 4 whole pixels, 4 * C bytes from a word boundary
        uint32_t w[NC];
#pragma unroll
        for (int j = 0; j < NC; ++j) w[j] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int e = i * NC + c;
                w[e >> 2] |= u[c][i] << ((e & 3) * 8);
            }
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int j = 0; j < NC; ++j) d4[j] = w[j];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < left) {
#pragma unroll
                for (int c = 0; c < NC; ++c) dst[i * NC + c] = (uint8_t)u[c][i];
            }
    }
}

const U8Table& u8_table() {
    static const U8Table tab = [] {
        U8Table t;
        for (int u = 0; u < 256; ++u) t.v[u] = (float)u / 255.0f;
        return t;
    }();
    return tab;
}

int popcount8(int mask) {
    int n = 0;
    for (int op = 0; op < 8; ++op) n += (mask >> op) & 1;
    return n;
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

}  // namespace

extern "C" int tdr_dihedral_gather(const void* src, int src_u8, int N, int C, int H, int W, int swap_rb, int ops_mask, float* out, void* stream) {
    TDR_REQUIRE(ops_mask > 0 && ops_mask < 256, "tdr_dihedral_gather: ops_mask 0x%x selects no op of 0 ... 7", ops_mask);
    TDR_REQUIRE((ops_mask & 0x0f) == 0 || (ops_mask & 0xf0) == 0, "tdr_dihedral_gather: ops_mask 0x%x mixes the straight ops (0 - 3) and the "
                "transposing ones (4 - 7): their outputs differ in shape, one call per class", ops_mask);
    TDR_REQUIRE(src && out, "tdr_dihedral_gather: null pointer");
    TDR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "tdr_dihedral_gather: bad sizes N %d, C %d, image %d x %d", N, C, H, W);
    TDR_REQUIRE(!src_u8 || C == 1 || C == 3 || C == 6, "tdr_dihedral_gather: %d byte channels (1, 3 or 6)", C);
    const int K = popcount8(ops_mask);
    const bool transposing = (ops_mask & 0xf0) != 0;
    const long units = (long)K * N * (src_u8 ? 1 : C);                 // planes (float source) / images (bytes) times ops
    const long blocks = transposing ? units * ((H + TS - 1) / TS) * ((W + TS - 1) / TS) : (units * H * ((W + 3) / 4) + 255) / 256;
    TDR_REQUIRE(blocks < (1L << 31), "tdr_dihedral_gather: %ld workgroups", blocks);
    const int Wo = transposing ? H : W;
    const int vec_dst = (Wo % 4 == 0) && aligned16(out);
    const int vec_src = (W % 4 == 0) && aligned16(src);
    const int word_src = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 4 == 0);
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
    if (!src_u8) {
        const float* f = (const float*)src;
        if (transposing) hipLaunchKernelGGL(dihedral_gather_transposed_f32_kernel, grid, block, 0, s, f, (long)N * C, H, W, ops_mask, out, vec_src, vec_dst);
        else hipLaunchKernelGGL(dihedral_gather_straight_f32_kernel, grid, block, 0, s, f, (long)N * C, H, W, ops_mask, K, out, vec_src, vec_dst);
        TDR_LAUNCH_CHECK("dihedral_gather_f32_kernel");
        return TDR_OK;
    }
    const uint8_t* img = (const uint8_t*)src;
    const U8Table& tab = u8_table();
    if (transposing) {
        if (C == 1) hipLaunchKernelGGL(dihedral_gather_transposed_u8_kernel<1>, grid, block, 0, s, img, N, H, W, swap_rb, ops_mask, out, word_src, vec_dst, tab);
        else if (C == 3) hipLaunchKernelGGL(dihedral_gather_transposed_u8_kernel<3>, grid, block, 0, s, img, N, H, W, swap_rb, ops_mask, out, word_src, vec_dst, tab);
        else hipLaunchKernelGGL(dihedral_gather_transposed_u8_kernel<6>, grid, block, 0, s, img, N, H, W, swap_rb, ops_mask, out, word_src, vec_dst, tab);
    } else {
        if (C == 1) hipLaunchKernelGGL(dihedral_gather_straight_u8_kernel<1>, grid, block, 0, s, img, N, H, W, swap_rb, ops_mask, K, out, word_src, vec_dst, tab);
        else if (C == 3) hipLaunchKernelGGL(dihedral_gather_straight_u8_kernel<3>, grid, block, 0, s, img, N, H, W, swap_rb, ops_mask, K, out, word_src, vec_dst, tab);
        else hipLaunchKernelGGL(dihedral_gather_straight_u8_kernel<6>, grid, block, 0, s, img, N, H, W, swap_rb, ops_mask, K, out, word_src, vec_dst, tab);
    }
    TDR_LAUNCH_CHECK("dihedral_gather_u8_kernel");
    return TDR_OK;
}

extern "C" int tdr_dihedral_mean(const float* straight, int mask_s, const float* transposed, int mask_t, int N, int C, int H, int W,
                                 float* out_f32, uint8_t* out_u8, int swap_rb, void* stream) {
    TDR_REQUIRE(mask_s >= 0 && (mask_s & ~0x0f) == 0 && mask_t >= 0 && (mask_t & ~0xf0) == 0, "tdr_dihedral_mean: mask_s 0x%x must lie in 0x0f "
                "(ops 0 - 3), mask_t 0x%x in 0xf0 (ops 4 - 7)", mask_s, mask_t);
    TDR_REQUIRE(mask_s || mask_t, "tdr_dihedral_mean: no op selected");
    TDR_REQUIRE((straight != nullptr) == (mask_s != 0) && (transposed != nullptr) == (mask_t != 0), "tdr_dihedral_mean: a member pointer goes with "
                "a non-empty mask, a null one with an empty mask (mask_s 0x%x, mask_t 0x%x)", mask_s, mask_t);
    TDR_REQUIRE((out_f32 != nullptr) != (out_u8 != nullptr), "tdr_dihedral_mean: exactly one of out_f32 and out_u8");
    TDR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0, "tdr_dihedral_mean: bad sizes N %d, C %d, image %d x %d", N, C, H, W);
    TDR_REQUIRE(!out_u8 || C == 1 || C == 3 || C == 6, "tdr_dihedral_mean: %d byte channels (1, 3 or 6)", C);
    const long blocks = (long)N * (out_u8 ? 1 : C) * ((H + TS - 1) / TS) * ((W + TS - 1) / TS);
    TDR_REQUIRE(blocks < (1L << 31), "tdr_dihedral_mean: %ld workgroups", blocks);
    const float count = (float)(popcount8(mask_s) + popcount8(mask_t));
    const int vec_s = (W % 4 == 0) && aligned16(straight), vec_t = (H % 4 == 0) && aligned16(transposed);
    const int vec_o = out_f32 ? (W % 4 == 0) && aligned16(out_f32) : (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out_u8) % 4 == 0);
    const dim3 grid((unsigned)blocks), block(256);
    hipStream_t s = (hipStream_t)stream;
#define TDR_DIHEDRAL_MEAN(CU8) hipLaunchKernelGGL(dihedral_mean_kernel<CU8>, grid, block, 0, s, straight, mask_s, transposed, mask_t, N, C, H, W, \
                                                  out_f32, out_u8, swap_rb, count, vec_s, vec_t, vec_o)
    if (out_f32) TDR_DIHEDRAL_MEAN(0);
    else if (C == 1) TDR_DIHEDRAL_MEAN(1);
    else if (C == 3) TDR_DIHEDRAL_MEAN(3);
    else TDR_DIHEDRAL_MEAN(6);
#undef TDR_DIHEDRAL_MEAN
    TDR_LAUNCH_CHECK("dihedral_mean_kernel");
    return TDR_OK;
}
