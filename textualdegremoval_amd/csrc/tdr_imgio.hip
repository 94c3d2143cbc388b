// Byte images in, byte images out -- the two host conversions of the reference's evaluation loop (utils/utils_image.py) on the device:
//   tdr_img_u8_to_planes : imfrombytes(float32=True) (:216-217, `img.astype(np.float32) / 255.`) + img2tensor(bgr2rgb) (:115-121) + the
//                          network's zero pad to (Hp, Wp):   uint8 [N][H][W][C] -> float32 [N][C][Hp][Wp]
//   tdr_planes_to_img_u8 : tensor2img(rgb2bgr, np.uint8, (0, 1)) (:160-187: clamp to [0, 1], `(img * 255.0).round()`, astype(uint8)) + the
//                          crop back to (H, W):              float32 [N][C][Hp][Wp] -> uint8 [N][H][W][C]
// Streaming kernels, one thread per 4 pixels of a row.  A plane row is read / written as one float4 where the row pitch and the base are
// 16-byte aligned and the 4 pixels lie inside it, pixel by pixel otherwise (odd widths, the last pixels of a row); the interleaved bytes
// of the 4 pixels move as C 32-bit words where W % 4 == 0 (the 4-pixel group then starts on a word), byte by byte otherwise.
// Number formats: float32(u) / 255.0f is read from a 256-entry table the host computes with that very division (IEEE, correctly rounded --
// numpy's); a product with the reciprocal does not round every value the same way.  The way back is float32 arithmetic as numpy's:
// fminf / fmaxf, one float32 product with 255.0f, rintf (round half to even, np.round's rule); the product is at most 255, so the cast is
// exact.  Like cv2.cvtColor in the reference, the red / blue swap applies to 3-channel images only.
#include "tdr_common.h"
#include "../../include/tdr.h"

#pragma clang fp contract(off)

namespace {

struct U8Table { float v[256]; };

template <int C>
__global__ __launch_bounds__(256) void u8_to_planes_kernel(const uint8_t* __restrict__ img, int N, int H, int W, int swap,
                                                           float* __restrict__ out, int Hp, int Wp, int vec, U8Table tab) {
    __shared__ float lut[256];
    lut[threadIdx.x] = tab.v[threadIdx.x];
    __syncthreads();
    const int groups = (Wp + 3) >> 2;
    const long total = (long)N * Hp * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % groups);
    const long row = t / groups;
    const int y = (int)(row % Hp), n = (int)(row / Hp), x0 = g << 2;
    float v[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int i = 0; i < 4; ++i) v[c][i] = 0.f;
    if (y < H && x0 < W) {
        const uint8_t* src = img + (((long)n * H + y) * W + x0) * C;
        if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 3) == 0) {      // 4 whole pixels, 4 * C bytes from a word boundary
            const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src);
            uint32_t w[C];
#pragma unroll
            for (int k = 0; k < C; ++k) w[k] = s4[k];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int b = i * C + c;
                    v[c][i] = lut[(w[b >> 2] >> ((b & 3) * 8)) & 0xff];
                }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < W) {
#pragma unroll
                    for (int c = 0; c < C; ++c) v[c][i] = lut[src[i * C + c]];
                }
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const int cr = C == 3 ? 2 - c : c;                     // swapped: plane c holds byte channel 2 - c
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (C == 3 && swap) ? v[cr][i] : v[c][i];
        float* dst = out + (((long)n * C + c) * Hp + y) * Wp + x0;
        if (vec && x0 + 3 < Wp) {
            *reinterpret_cast<float4*>(dst) = make_float4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (x0 + i < Wp) dst[i] = o[i];
        }
    }
}

__device__ __forceinline__ uint32_t to_u8(float x) {
    x = fminf(fmaxf(x, 0.f), 1.f);
    return (uint32_t)rintf(x * 255.0f);
}

template <int C>
__global__ __launch_bounds__(256) void planes_to_u8_kernel(const float* __restrict__ in, int N, int Hp, int Wp, int swap,
                                                           uint8_t* __restrict__ img, int H, int W, int vec) {
    const int groups = (W + 3) >> 2;
    const long total = (long)N * H * groups;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int g = (int)(t % groups);
    const long row = t / groups;
    const int y = (int)(row % H), n = (int)(row / H), x0 = g << 2;
    uint32_t q[C][4];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float* src = in + (((long)n * C + c) * Hp + y) * Wp + x0;
        if (vec && x0 + 3 < Wp) {                                // (pixels past W but inside the padded row are read and dropped)
            const float4 f = *reinterpret_cast<const float4*>(src);
            q[c][0] = to_u8(f.x); q[c][1] = to_u8(f.y); q[c][2] = to_u8(f.z); q[c][3] = to_u8(f.w);
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) q[c][i] = (x0 + i < W) ? to_u8(src[i]) : 0u;
        }
    }
    uint8_t* dst = img + (((long)n * H + y) * W + x0) * C;
    if ((W & 3) == 0 && (reinterpret_cast<uintptr_t>(img) & 3) == 0) {
        uint32_t w[C];
#pragma unroll
        for (int k = 0; k < C; ++k) w[k] = 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const int b = i * C + c;
                w[b >> 2] |= ((C == 3 && swap) ? q[C == 3 ? 2 - c : c][i] : q[c][i]) << ((b & 3) * 8);
            }
        uint32_t* d4 = reinterpret_cast<uint32_t*>(dst);
#pragma unroll
        for (int k = 0; k < C; ++k) d4[k] = w[k];
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x0 + i < W) {
#pragma unroll
                for (int c = 0; c < C; ++c) dst[i * C + c] = (uint8_t)((C == 3 && swap) ? q[C == 3 ? 2 - c : c][i] : q[c][i]);
            }
    }
}

int check_dims(const char* fn, int N, int H, int W, int C, int Hp, int Wp, long* blocks, int out_rows, int out_cols) {
    TDR_REQUIRE(N > 0 && H > 0 && W > 0 && Hp >= H && Wp >= W, "%s: bad sizes N %d, image %d x %d, planes %d x %d", fn, N, H, W, Hp, Wp);
    TDR_REQUIRE(C == 1 || C == 3 || C == 6, "%s: %d channels (1, 3 or 6)", fn, C);
    const long threads = (long)N * out_rows * ((out_cols + 3) / 4);
    *blocks = (threads + 255) / 256;
    TDR_REQUIRE(*blocks < (1L << 31), "%s: %ld workgroups", fn, *blocks);
    return TDR_OK;
}

}  // namespace

extern "C" int tdr_img_u8_to_planes(const uint8_t* img, int N, int H, int W, int C, int swap_rb, float* out, int Hp, int Wp, void* stream) {
    TDR_REQUIRE(img && out, "tdr_img_u8_to_planes: null pointer");
    long blocks = 0;
    if (int rc = check_dims("tdr_img_u8_to_planes", N, H, W, C, Hp, Wp, &blocks, Hp, Wp)) return rc;
    static const U8Table tab = [] {
        U8Table t;
        for (int u = 0; u < 256; ++u) t.v[u] = (float)u / 255.0f;
        return t;
    }();
    const int vec = (Wp % 4 == 0) && (reinterpret_cast<uintptr_t>(out) % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    if (C == 1) hipLaunchKernelGGL(u8_to_planes_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, img, N, H, W, swap_rb, out, Hp, Wp, vec, tab);
    else if (C == 3) hipLaunchKernelGGL(u8_to_planes_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, s, img, N, H, W, swap_rb, out, Hp, Wp, vec, tab);
    else hipLaunchKernelGGL(u8_to_planes_kernel<6>, dim3((unsigned)blocks), dim3(256), 0, s, img, N, H, W, swap_rb, out, Hp, Wp, vec, tab);
    TDR_LAUNCH_CHECK("u8_to_planes_kernel");
    return TDR_OK;
}

extern "C" int tdr_planes_to_img_u8(const float* in, int N, int C, int Hp, int Wp, int swap_rb, uint8_t* img, int H, int W, void* stream) {
    TDR_REQUIRE(in && img, "tdr_planes_to_img_u8: null pointer");
    long blocks = 0;
    if (int rc = check_dims("tdr_planes_to_img_u8", N, H, W, C, Hp, Wp, &blocks, H, W)) return rc;
    const int vec = (Wp % 4 == 0) && (reinterpret_cast<uintptr_t>(in) % 16 == 0);
    hipStream_t s = (hipStream_t)stream;
    if (C == 1) hipLaunchKernelGGL(planes_to_u8_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, in, N, Hp, Wp, swap_rb, img, H, W, vec);
    else if (C == 3) hipLaunchKernelGGL(planes_to_u8_kernel<3>, dim3((unsigned)blocks), dim3(256), 0, s, in, N, Hp, Wp, swap_rb, img, H, W, vec);
    else hipLaunchKernelGGL(planes_to_u8_kernel<6>, dim3((unsigned)blocks), dim3(256), 0, s, in, N, Hp, Wp, swap_rb, img, H, W, vec);
    TDR_LAUNCH_CHECK("planes_to_u8_kernel");
    return TDR_OK;
}
