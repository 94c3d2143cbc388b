// Forward-only second half of a NAFBlock under TLSC (models/archs/nafnet_local_arch.py:10-104, `NAFNetLocal`): the SCA statistic is a
// box mean MAP instead of one number per plane, so the channel attention is a per-pixel GEMM of its own in front of conv3:
//
//     s   = W_sca boxmean(g) + b_sca                     (boxmean: tdr_local_avgpool, csrc/tdr_tlsc.hip)
//     y   = inp + conv3(g * s) * beta
//     out = y + conv5(SimpleGate(conv4(norm2(y)))) * gamma
//
// tdr_naf_tail_infer_local is naf_tail_fwd_kernel<C, KEEP = false> of tdr_nafblock_chain.h -- tile (64 pixels x all channels, 2C threads,
// wave w owns rows [32w, 32w + 32)), LDS planes, `red` buffer, group rotation, both split schemes -- with ONE phase in front: the pooled
// tile is staged into the planes, W_sca runs over it like conv3 does (same fragment layout), the accumulators plus b_sca are s in
// accumulator layout, and g * s (g read in that layout too) goes back into the planes as conv3's operand.  From conv3 on the kernel is
// the forward-only tail.  A kernel of its own, built from the header's helpers: the header's kernels are not touched, so the code of
// the other three units stays what it was (profiles/probe_infer_isa.py).
// Registers: the residual tile is requested AFTER the phase -- during it the live set is the g tile and one accumulator tile, what the
// conv3 phase holds with the residual tile (C = 256 sits at the 256-VGPR limit of two waves per SIMD).
#include "tdr_nafblock_chain.h"

namespace {

struct TailLocalArgs {
    const float* g; long g_ns;
    const float* pool; long pool_ns;  // box mean of g, [N][C][HW]
    const float* x; long x_ns;
    const uint4 *wsca, *w3, *w4, *w5; // packed fragments (PACK_FWD): M = C, C, 2C, C; K = C
    const float *bsca, *b3, *beta, *lnw, *lnb, *b4, *b5, *gamma;
    float eps;
    float* out; long out_ns;
    int HW;
};

template <int C, int SCH>
__global__ __launch_bounds__(2 * C, 2) void naf_tail_local_kernel(TailLocalArgs a) {
    static_assert(C == 256 || C == 128 || C == 64 || C == 32, "C / 32 waves x 32 channel rows");
    constexpr int NS = SchT<SCH>::NS;
    constexpr int NOCT = C / 8;               // octets of the K = C operands
    constexpr int NG = C / 16;
    constexpr int NW = C / 32;
    extern __shared__ __attribute__((aligned(16))) uint4 smem4[];
    uint4* sB = smem4;                                        // NS planes x NOCT x 64 px x 16 B
    float* red = reinterpret_cast<float*>(smem4 + NS * NOCT * NPX);   // [2][NW][64 px]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31, kk = lane >> 5;
    const int n = blockIdx.y;
    const long p0 = (long)blockIdx.x * NPX;
    const long HW = a.HW;
    const int m0 = 32 * wave;                                 // first channel row of this wave
    const int rot = (int)(blockIdx.x * 5);
    auto off = [&](int r, int tn) { return (long)(m0 + row_of(r, kk)) * HW + 32 * tn; };

    // ---- stage B = boxmean(g): thread (oct, q) owns pixels 4q..4q+3 of octet oct
    {
        const int q = tid & 15, oct = tid >> 4;
        const float* pp = a.pool + (long)n * a.pool_ns + p0 + 4 * q;
        const float one8[8] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
        float4 v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = *reinterpret_cast<const float4*>(pp + (long)(8 * oct + i) * HW);
        stage_octet<SCH, false>(v, one8, sB, NOCT, oct, q);
    }
    // ---- the g tile of this wave's rows in accumulator layout: requested ahead of the GEMM that produces its partner
    float gv[2][16];
    {
        const float* gp = a.g + (long)n * a.g_ns + p0 + j;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) gv[tn][r] = gp[off(r, tn)];
    }
    __syncthreads();

    // ---- sca: s = W_sca boxmean(g) + b_sca ; conv3's operand g * s
    f32x16 acc[1][2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][tn][r] = 0.f;
    gemm_split<SCH, 1, NG, 2>(acc, a.wsca, C / 32, [&](int) { return wave; }, sB, NOCT, lane, rot, [](int) {});
    {
        float bsv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) bsv[r] = a.bsca[m0 + row_of(r, kk)];
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) gv[tn][r] *= acc[0][tn][r] + bsv[r];
    }
    __syncthreads();                                          // every wave has finished reading the pooled planes
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) tile_to_planes<SCH>(gv[tn], sB, NOCT, 4 * wave, 32 * tn + j, kk);

    // ---- residual tile (inp) in accumulator layout: requested here, consumed after conv3
    float xr[2][16];
    {
        const float* xp = a.x + (long)n * a.x_ns + p0 + j;
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) xr[tn][r] = xp[off(r, tn)];
    }
    float b3v[16], bev[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        b3v[r] = a.b3[m0 + row_of(r, kk)];
        bev[r] = a.beta[m0 + row_of(r, kk)];
    }
    __syncthreads();

    // ---- from here on: naf_tail_fwd_kernel<C, KEEP = false>.  conv3: y = (W3 (g*s) + b3) * beta + inp
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][tn][r] = 0.f;
    gemm_split<SCH, 1, NG, 2>(acc, a.w3, C / 32, [&](int) { return wave; }, sB, NOCT, lane, rot, [](int) {});

    float yv[2][16];
    float psum[2] = {0.f, 0.f};
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float v = (acc[0][tn][r] + b3v[r]) * bev[r] + xr[tn][r];
            yv[tn][r] = v;
            psum[tn] += v;
        }
    // ---- norm2: mean, then centred second moment (two passes over the register tile)
    float mean[2], rstd[2];
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        psum[tn] += __shfl_xor(psum[tn], 32, 64);
        if (kk == 0) red[wave * NPX + 32 * tn + j] = psum[tn];
    }
    __syncthreads();                                          // (all waves are past their conv3 reads of sB here)
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) mean[tn] = wave_partials_sum<NW>(red + 32 * tn + j) * (1.f / C);
    float pvar[2] = {0.f, 0.f};
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float d = yv[tn][r] - mean[tn];
            pvar[tn] += d * d;
        }
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        pvar[tn] += __shfl_xor(pvar[tn], 32, 64);
        if (kk == 0) red[(NW + wave) * NPX + 32 * tn + j] = pvar[tn];
    }
    __syncthreads();
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const float var = wave_partials_sum<NW>(red + NW * NPX + 32 * tn + j) * (1.f / C);
        rstd[tn] = 1.f / sqrtf(var + a.eps);
    }
    // yn = (y - mu) * rstd * w + b, split into the LDS operand
    {
        float lw[16], lb[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            lw[r] = a.lnw[m0 + row_of(r, kk)];
            lb[r] = a.lnb[m0 + row_of(r, kk)];
        }
#pragma unroll
        for (int tn = 0; tn < 2; ++tn) {
            float ynv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) ynv[r] = (yv[tn][r] - mean[tn]) * rstd[tn] * lw[r] + lb[r];
            tile_to_planes<SCH>(ynv, sB, NOCT, 4 * wave, 32 * tn + j, kk);
        }
    }
    __syncthreads();

    // ---- conv4: t4 = W4 yn + b4 ; rows [32w, 32w+32) and their gate partners [C + 32w, C + 32w + 32)
    f32x16 acc4[2][2];
#pragma unroll
    for (int tm = 0; tm < 2; ++tm)
#pragma unroll
        for (int tn = 0; tn < 2; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc4[tm][tn][r] = 0.f;
    gemm_split<SCH, 2, NG, 2>(acc4, a.w4, 2 * C / 32, [&](int tm) { return tm * (C / 32) + wave; }, sB, NOCT, lane, rot, [](int) {});
    {
        float b4v[2][16];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) b4v[tm][r] = a.b4[tm * C + m0 + row_of(r, kk)];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < 2; ++tn)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc4[tm][tn][r] += b4v[tm][r];
    }
    __syncthreads();                                          // every wave has finished reading the yn planes
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        float v[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = acc4[0][tn][r] * acc4[1][tn][r];      // SimpleGate (:170-175)
        tile_to_planes<SCH>(v, sB, NOCT, 4 * wave, 32 * tn + j, kk);
    }
    float b5v[16], gav[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        b5v[r] = a.b5[m0 + row_of(r, kk)];
        gav[r] = a.gamma[m0 + row_of(r, kk)];
    }
    __syncthreads();

    // ---- conv5: out = (W5 gate + b5) * gamma + y
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[0][tn][r] = 0.f;
    gemm_split<SCH, 1, NG, 2>(acc, a.w5, C / 32, [&](int) { return wave; }, sB, NOCT, lane, rot, [](int) {});
    float* op = a.out + (long)n * a.out_ns + p0 + j;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn)
#pragma unroll
        for (int r = 0; r < 16; ++r) op[off(r, tn)] = (acc[0][tn][r] + b5v[r]) * gav[r] + yv[tn][r];
}

}  // namespace

extern "C" int tdr_naf_tail_infer_local(const TdrNafTailLocalDesc* d, void* stream) {
    const char* fn = "tdr_naf_tail_infer_local";
    TDR_REQUIRE(d && d->g && d->pool && d->x && d->wsca && d->w3 && d->w4 && d->w5 && d->bsca && d->b3 && d->beta && d->lnw && d->lnb &&
                    d->b4 && d->b5 && d->gamma && d->out,
                "%s: null pointer", fn);
    TDR_REQUIRE(d->N >= 1 && naf_chain_supported(d->C, d->HW), "%s: needs C in {32, 64, 128, 256} and HW %% 64 == 0 (got N=%d C=%d HW=%d)", fn,
                d->N, d->C, d->HW);
    TDR_REQUIRE(d->w_fmt == 2 || d->w_fmt == 1, "%s: weights must be packed with tdr_pack_weights_hx2 / _bx3 (mode FWD)", fn);
    TDR_REQUIRE(d->pool_ns % 4 == 0 && (reinterpret_cast<uintptr_t>(d->pool) & 15) == 0, "%s: pool must be 16-byte aligned", fn);
    TailLocalArgs a;
    a.g = d->g; a.g_ns = d->g_ns; a.pool = d->pool; a.pool_ns = d->pool_ns; a.x = d->x; a.x_ns = d->x_ns;
    a.wsca = reinterpret_cast<const uint4*>(d->wsca); a.w3 = reinterpret_cast<const uint4*>(d->w3);
    a.w4 = reinterpret_cast<const uint4*>(d->w4); a.w5 = reinterpret_cast<const uint4*>(d->w5);
    a.bsca = d->bsca; a.b3 = d->b3; a.beta = d->beta; a.lnw = d->lnw; a.lnb = d->lnb; a.b4 = d->b4; a.b5 = d->b5; a.gamma = d->gamma;
    a.eps = d->eps; a.out = d->out; a.out_ns = d->out_ns; a.HW = d->HW;
    const bool bx = d->w_fmt == 1;
    NAF_DISPATCH_CS(naf_tail_local_kernel, , , naf_fwd_lds_bytes(d->C, bx), a, d, stream);
    TDR_LAUNCH_CHECK("naf_tail_local_kernel");
    return TDR_OK;
}
