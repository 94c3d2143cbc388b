// Tiled inference (inference.InferenceSession.run_tiled): the two passes around the network when an image of any size runs through the
// graph of one tile shape.
//   tdr_tile_gather      : one batch of tiles out of the images, a device table of (n, y0, x0) per tile:
//                          float32 [N][C][H][W] or uint8 [N][H][W][C]  ->  float32 [B][C][th][tw]
//   tdr_tile_blend       : the output images from all tile outputs of the call, a weighted sum over the tiles that cover a pixel:
//                          float32 [N * ny * nx][C][th][tw]  ->  float32 [N][C][H][W]
// Streaming kernels in the style of tdr_imgio.hip, one thread per 4 pixels of a row: a float4 where base, pitch and the tile's column are
// 16-byte aligned and the 4 pixels lie inside the row, pixel by pixel otherwise; interleaved bytes as C 32-bit words where the 4-pixel
// group starts on a word.  The byte source goes through the 256-entry float32(u) / 255.0f table of tdr_img_u8_to_planes (the same
// division, computed on the host), so a gathered tile holds the bits of the corresponding slice of that kernel's planes.
// The blend is a gather -- no atomics, no accumulation buffer: per pixel the terms are added in a fixed order, (wy[a] * wx[b]) * v with
// a outside and b inside, fp32 without contraction.  The sum starts from -0.0f, the one value that leaves every first term as it is
// (+0 and -0 included): a pixel covered once, weight 1.0f, is a bit-exact copy.
// The tables live in device memory, out of the host's sight: a gather entry that does not lie inside its image yields a tile of zeros, a
// blend term whose tile or offset is out of range is left out -- neither kernel reads outside what the sizes passed by value describe.
#include "tdr_common.h"
#include "../../include/tdr.h"

#pragma clang fp contract(off)

namespace {

struct U8Table { float v[256]; };

__device__ __forceinline__ bool tile_inside(int n, int y0, int x0, int N, int H, int W, int th, int tw) {
    return n >= 0 && n < N && y0 >= 0 && x0 >= 0 && y0 <= H - th && x0 <= W - tw;
}

__global__ __launch_bounds__(256) void tile_gather_f32_kernel(const float* __restrict__ src, int N, int C, int H, int W,
                                                              const int* __restrict__ table, int B, int th, int tw,
                                                              float* __restrict__ out, int vec_src, int vec_dst) {
    const int groups = (tw + 3) >> 2;
    const long total = (long)B * C * th * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % groups);
    long row = t / groups;
    const int y = (int)(row % th);
    row /= th;
    const int c = (int)(row % C), b = (int)(row / C), x = g << 2;
    const int n = table[b * 3], y0 = table[b * 3 + 1], x0 = table[b * 3 + 2];
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    if (tile_inside(n, y0, x0, N, H, W, th, tw)) {
        const float* s = src + (((long)n * C + c) * H + y0 + y) * W + x0 + x;
        if (vec_src && (x0 & 3) == 0 && x + 3 < tw) {
            const float4 f = *reinterpret_cast<const float4*>(s);
            o[0] = f.x; o[1] = f.y; o[2] = f.z; o[3] = f.w;
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < tw) o[i] = s[i];
        }
    }
    float* dst = out + (((long)b * C + c) * th + y) * tw + x;
    if (vec_dst && x + 3 < tw) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < tw) dst[i] = o[i];
    }
}

template <int C>
__global__ __launch_bounds__(256) void tile_gather_u8_kernel(const uint8_t* __restrict__ img, int N, int H, int W, int swap,
                                                             const int* __restrict__ table, int B, int th, int tw,
                                                             float* __restrict__ out, int word_src, int vec_dst, U8Table tab) {
    __shared__ float lut[256];
    lut[threadIdx.x] = tab.v[threadIdx.x];
    __syncthreads();
    const int groups = (tw + 3) >> 2;
    const long total = (long)B * th * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % groups);
    const long row = t / groups;
    const int y = (int)(row % th), b = (int)(row / th), x = g << 2;
    const int n = table[b * 3], y0 = table[b * 3 + 1], x0 = table[b * 3 + 2];
    float v[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = 0.f;
    if (tile_inside(n, y0, x0, N, H, W, th, tw)) {
        const uint8_t* s = img + (((long)n * H + y0 + y) * W + x0 + x) * C;
        if (word_src && (x0 & 3) == 0 && x + 3 < tw) {                 // 4 whole pixels, 4 * C bytes from a word boundary
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(s);
            uint32_t w[C];
#pragma unroll
            for (int k = 0; k < C; ++k) w[k] = s4[k];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int q = i * C + c;
                    v[c][i] = lut[(w[q >> 2] >> ((q & 3) * 8)) & 0xff];
                }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < tw) {
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c][i] = lut[s[i * C + c]];
                }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int cr = C == 3 ? 2 - c : c;                             // swapped: plane c holds byte channel 2 - c
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (C == 3 && swap) ? v[cr][i] : v[c][i];
        float* dst = out + (((long)b * C + c) * th + y) * tw + x;
        if (vec_dst && x + 3 < tw) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x + i < tw) dst[i] = o[i];
        }
    }
}

// the tables of one dimension: start[n_tiles]; idx[L][2] = (first covering tile, how many); w[L][K] their weights
struct TileDim {
    const int* start;
    const int* idx;
    const float* w;
    int K, n, t;
};

__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, int N, int C, int H, int W, TileDim ty, TileDim tx,
                                                         float* __restrict__ out, int vec_src, int vec_dst) {
    const int groups = (W + 3) >> 2;
    const long total = (long)N * C * H * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % groups);
    long row = t / groups;
    const int y = (int)(row % H);
    row /= H;
    const int c = (int)(row % C), n = (int)(row / C), x = g << 2;
    const int fy = ty.idx[2 * y], cy = min(ty.idx[2 * y + 1], ty.K);
    const long plane = (long)ty.t * tx.t;
    float o[4] = {-0.f, -0.f, -0.f, -0.f};
    // 4 pixels under one tile column, covered once, from a 16-byte boundary of the tile's row: one float4 per covering tile row
    bool one = false;
    int fx0 = 0, xs0 = 0;
    if (x + 3 < W) {
        fx0 = tx.idx[2 * x];
        one = tx.idx[2 * x + 1] == 1 && tx.idx[2 * x + 3] == 1 && tx.idx[2 * x + 5] == 1 && tx.idx[2 * x + 7] == 1 &&
              tx.idx[2 * x + 2] == fx0 && tx.idx[2 * x + 4] == fx0 && tx.idx[2 * x + 6] == fx0 && fx0 >= 0 && fx0 < tx.n;
        if (one) {
            xs0 = tx.start[fx0];
            one = x - xs0 >= 0 && x - xs0 + 3 < tx.t;
        }
    }
    if (one) {
        const float wx0 = tx.w[(long)x * tx.K], wx1 = tx.w[(long)(x + 1) * tx.K], wx2 = tx.w[(long)(x + 2) * tx.K], wx3 = tx.w[(long)(x + 3) * tx.K];
        for (int a = 0; a < cy; ++a) {
            const int iy = fy + a;
            if (iy < 0 || iy >= ty.n) continue;
            const int oy = y - ty.start[iy];
            if (oy < 0 || oy >= ty.t) continue;
            const float wy = ty.w[(long)y * ty.K + a];
            const float* s = tiles + ((((long)n * ty.n + iy) * tx.n + fx0) * C + c) * plane + (long)oy * tx.t + (x - xs0);
            float f[4];
            if (vec_src && ((x - xs0) & 3) == 0) {
                const float4 q = *reinterpret_cast<const float4*>(s);
                f[0] = q.x; f[1] = q.y; f[2] = q.z; f[3] = q.w;
            } else {
                f[0] = s[0]; f[1] = s[1]; f[2] = s[2]; f[3] = s[3];
            }
            o[0] = o[0] + (wy * wx0) * f[0];
            o[1] = o[1] + (wy * wx1) * f[1];
            o[2] = o[2] + (wy * wx2) * f[2];
            o[3] = o[3] + (wy * wx3) * f[3];
        }
    } else {
        for (int a = 0; a < cy; ++a) {
            const int iy = fy + a;
            if (iy < 0 || iy >= ty.n) continue;
            const int oy = y - ty.start[iy];
            if (oy < 0 || oy >= ty.t) continue;
            const float wy = ty.w[(long)y * ty.K + a];
            const float* srow = tiles + ((long)n * ty.n + iy) * tx.n * C * plane + (long)c * plane + (long)oy * tx.t;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (x + i >= W) continue;
                const int fx = tx.idx[2 * (x + i)], cx = min(tx.idx[2 * (x + i) + 1], tx.K);
                for (int b = 0; b < cx; ++b) {
                    const int ix = fx + b;
                    if (ix < 0 || ix >= tx.n) continue;
                    const int ox = x + i - tx.start[ix];
                    if (ox < 0 || ox >= tx.t) continue;
                    o[i] = o[i] + (wy * tx.w[(long)(x + i) * tx.K + b]) * srow[(long)ix * C * plane + ox];
                }
            }
        }
    }
    float* dst = out + (((long)n * C + c) * H + y) * W + x;
    if (vec_dst && x + 3 < W) {
        *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x + i < W) dst[i] = o[i];
    }
}

}  // namespace

extern "C" int tdr_tile_gather(const void* src, int src_u8, int N, int C, int H, int W, int swap_rb, const int* table, int B, int th, int tw,
                               float* out, void* stream) {
    TDR_REQUIRE(src && table && out, "tdr_tile_gather: null pointer");
    TDR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && B > 0, "tdr_tile_gather: bad sizes N %d, C %d, image %d x %d, %d tiles", N, C, H, W, B);
    TDR_REQUIRE(th > 0 && tw > 0 && th <= H && tw <= W, "tdr_tile_gather: a %d x %d tile does not lie inside a %d x %d image", th, tw, H, W);
    TDR_REQUIRE(!src_u8 || C == 1 || C == 3 || C == 6, "tdr_tile_gather: %d byte channels (1, 3 or 6)", C);
    const long threads = (long)B * (src_u8 ? 1 : C) * th * ((tw + 3) / 4);
    const long blocks = (threads + 255) / 256;
    TDR_REQUIRE(blocks < (1L << 31), "tdr_tile_gather: %ld workgroups", blocks);
    const int vec_dst = (tw % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    if (!src_u8) {
        const int vec_src = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 16 == 0);
        hipLaunchKernelGGL(tile_gather_f32_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const float*)src, N, C, H, W, table, B, th, tw, out,
                           vec_src, vec_dst);
        TDR_LAUNCH_CHECK("tile_gather_f32_kernel");
        return TDR_OK;
    }
    static const U8Table tab = [] {
        U8Table t;
        for (int u = 0; u < 256; ++u) t.v[u] = (float)u / 255.0f;
        return t;
    }();
    const uint8_t* img = (const uint8_t*)src;
    const int word_src = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(src) % 4 == 0);
    if (C == 1) hipLaunchKernelGGL(tile_gather_u8_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, img, N, H, W, swap_rb, table, B, th, tw, out, word_src, vec_dst, tab);
    else if (C == 3) hipLaunchKernelGGL(tile_gather_u8_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, s, img, N, H, W, swap_rb, table, B, th, tw, out, word_src, vec_dst, tab);
    else hipLaunchKernelGGL(tile_gather_u8_kernel<6>, dim3((unsigned)blocks), dim3(256), 0, s, img, N, H, W, swap_rb, table, B, th, tw, out, word_src, vec_dst, tab);
    TDR_LAUNCH_CHECK("tile_gather_u8_kernel");
    return TDR_OK;
}

extern "C" int tdr_tile_blend(const float* tiles, int N, int C, int H, int W, int th, int tw, int ny, int nx, const int* ystart,
                              const int* yidx, const float* yw, int Ky, const int* xstart, const int* xidx, const float* xw, int Kx,
                              float* out, void* stream) {
    TDR_REQUIRE(tiles && ystart && yidx && yw && xstart && xidx && xw && out, "tdr_tile_blend: null pointer");
    TDR_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && ny > 0 && nx > 0 && Ky > 0 && Kx > 0, "tdr_tile_blend: bad sizes N %d, C %d, image %d x %d, "
                "%d x %d tiles, table widths %d, %d", N, C, H, W, ny, nx, Ky, Kx);
    TDR_REQUIRE(th > 0 && tw > 0 && th <= H && tw <= W, "tdr_tile_blend: a %d x %d tile does not lie inside a %d x %d image", th, tw, H, W);
    TDR_REQUIRE((long)ny * th >= H && (long)nx * tw >= W, "tdr_tile_blend: %d x %d tiles of %d x %d cannot cover a %d x %d image", ny, nx, th, tw, H, W);
    const long threads = (long)N * C * H * ((W + 3) / 4);
    const long blocks = (threads + 255) / 256;
    TDR_REQUIRE(blocks < (1L << 31), "tdr_tile_blend: %ld workgroups", blocks);
    const TileDim ty = {ystart, yidx, yw, Ky, ny, th}, tx = {xstart, xidx, xw, Kx, nx, tw};
    const int vec_src = (tw % 4 == 0) && (reinterpret_cast<uintptr_t>(tiles) % 16 == 0);
    const int vec_dst = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, tiles, N, C, H, W, ty, tx, out, vec_src, vec_dst);
    TDR_LAUNCH_CHECK("tile_blend_kernel");
    return TDR_OK;
}
