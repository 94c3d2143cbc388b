// Weight gradient of the 3x3 / stride 1 / pad 1 convolutions on PRE-SPLIT operands (P16 tensors, see tdr_conv_p16.hip), gfx950.
//
//   G[co][ci][ky][kx] = sum_{n,y,x} dout[n][co][y][x] * in[n][ci][y+ky-1][x+kx-1]
//
// MFMA view (v_mfma_f32_32x32x16_f16, 2-way fp16 split: products mh, hm, hh, fp32 accumulation): A[i = co][k = pixel],
// B[k = pixel][j = ci], one 32x32 accumulator per tap.  The contraction runs over PIXELS while a P16 slot holds 8 CHANNELS of one
// pixel -- the transposition the fp32 kernel (tdr_wgrad_bx3.hip) did with global loads of 8 consecutive pixels per lane, an
// operand split per element and v_alignbit assembly of the shifted fragments (VALU issue time ~ MFMA time) is done here by the
// LDS itself: ds_read_b64_tr_b16 hands lane n of a 16-lane group element n%4 of the 8 bytes lane 4e + n/4 pointed at
// (profiles/probes/tr16_probe.hip), so with lane s of a group pointing at pixel s/4, channels 4*(s%4).. of the tile, lane n
// receives channel n of four consecutive pixels: an MFMA operand fragment is two such reads, any tap shift is an address
// offset (slots are per pixel), and no VALU instruction touches an operand.
//
// A workgroup owns a (co-tile, ci-tile) pair and walks down a 32-column strip of one image: per step of RS rows it LDS-DMAs
// RS new input rows (+2 halo rows at the top of its chunk) and RS gradient rows into row rings ([octet][plane][column]
// slots, lane-linear), runs 2*RS k-steps of 27 MFMAs per wave (+2 against a fragment of ones for the bias gradient), one
// barrier per step.  Split-K partials [split][co][ci][9] are reduced in fixed order by wgrad_p16_reduce_kernel: deterministic.
//
// Grouped form (tdr_wgrad3x3_p16_group): the problems of ONE shape -- the 8 ResidualBlock convolutions of an encoder level -- share a
// launch.  A problem's K is its N x strips x chunks units in (n, strip, chunk) order; a workgroup owns one (problem, output tile, slice)
// and walks a contiguous, balanced run of units (per unit: halo rows, prologue barrier, row loop -- what one workgroup of the
// single-problem launch does) with its nine accumulators and the bias accumulator kept across units.  The same 512 workgroups that one
// problem cut into 512 / 512 / 128 / 32 / 8 slices at C = 32 .. 512 now need 64 / 64 / 16 / 4 / 1 slices per problem: 1 / 8 of the
// partial volume, one table-driven reduction launch per level, and with one slice the workgroup writes g / db itself (no workspace,
// no reduction).  1-D grid: block r of a chunk of 8 T blocks (T = output tiles) is tile r / 8 of (problem, slice) pair r % 8, so the
// tiles of a pair sit on one XCD and share their operand rows in its L2 (as wgrad1x1_sp_kernel<GRP>); nothing depends on placement.
//
// Replaces (reference): autograd's weight / bias gradient of the ResidualBlock convolutions of the MASA encoder
// (models/archs/network_nafnet_guided_arch.py:44-59,110-143).
#include <stdlib.h>
#include <stdint.h>
#include "tdr_common.h"
#include "../../include/tdr.h"

typedef _Float16 wf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 wbf16x8 __attribute__((ext_vector_type(8)));
typedef short ws16x4 __attribute__((ext_vector_type(4)));
typedef short ws16x8 __attribute__((ext_vector_type(8)));

namespace {

struct WgP16Args {
    const uint4* in; const uint4* dout;       // P16 tensors
    int Cin, Cout, H, W, Hp, Wp;
    int strips, chunks, rc;                    // 32-column strips per image, row chunks per strip, rows per chunk
    float* part; float* dbpart;
    // grouped launch (tdr_wgrad3x3_p16_group): TdrWg1GroupEntry[] in device memory, (problem, slice) pairs, slices per problem, units
    // (= N * strips * chunks) per problem, output tiles along co / ci
    const void* grp_tab; int grp_pairs, grp_nsplit, grp_units, tiles_co, tiles_ci;
};

#define WGP_GLDS(gptr, lptr)                                                                          \
    __builtin_amdgcn_global_load_lds((__attribute__((address_space(1))) const void*)(gptr),          \
                                     (__attribute__((address_space(3))) void*)(lptr), 16, 0, 0)

__device__ __forceinline__ ws16x8 tr_frag(const char* p, int off0, int off1) {
    const ws16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ws16x4*)(p + off0));
    const ws16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) ws16x4*)(p + off1));
    const ws16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return v;
}
// one matrix product of two 16-bit fragments: fp16 (pair planes) or bf16 (triple planes)
template <int NS>
__device__ __forceinline__ f32x16 wg_mfma(ws16x8 x, ws16x8 y, f32x16 c) {
    if constexpr (NS == 3) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(wbf16x8, x), __builtin_bit_cast(wbf16x8, y), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(wf16x8, x), __builtin_bit_cast(wf16x8, y), c, 0, 0, 0);
}

// WM x WN x WK = 4 waves; wave (wm, wn) owns the 32 co x 32 ci tile pair, WK waves share it and split the k-steps of a step.
// NS: planes of the operand tensors (2: fp16 pair, products mh hm hh; 3: bf16 triple, products lh hl mm mh hm hh -- the plane
// formats of tdr_conv_p16.hip).
// GRP: the grouped form (see the header); false: blockIdx = (unit, co tile, ci tile), one unit per workgroup.
template <int WM, int WN, int WK, int NS = 2, bool GRP = false>
__global__ __launch_bounds__(256, 2) void wgrad3x3_p16_kernel(WgP16Args a) {
    static_assert(WM * WN * WK == 4, "4 waves");
    constexpr int RS = WK == 4 ? 2 : 1;                  // rows per step (2 k-steps of 16 pixels per row)
    static_assert(2 * RS % WK == 0, "k-steps of a step split evenly over the K waves");
    constexpr int BMo = 32 * WM, BNi = 32 * WN, NOo = BMo / 8, NOi = BNi / 8;
    constexpr int XS = 2 * RS + 2, DS = 2 * RS;          // ring slots (rows)
    constexpr int XR = ((NOi * NS * 34 + 63) / 64) * 64; // slots per input row (padded to whole pieces)
    constexpr int DR = NOo * NS * 32;                    // slots per gradient row
    constexpr int XP = XR / 64, DP = DR / 64;            // pieces per row

    extern __shared__ __attribute__((aligned(1024))) uint4 smem4[];
    uint4* sX = smem4;                  // [XS][XR]
    uint4* sD = smem4 + XS * XR;        // [DS][DR]

    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wk = wave % WK, wn = (wave / WK) % WN, wm = wave / (WK * WN);
    int split = blockIdx.x, u0 = blockIdx.x, u1 = u0 + 1, tco = blockIdx.y, tci = blockIdx.z;
    float* dbout = a.dbpart;
    if constexpr (GRP) {
        const int T = a.tiles_co * a.tiles_ci;
        const int c8 = (int)blockIdx.x / (8 * T), r = (int)blockIdx.x - c8 * (8 * T);
        const int pair = c8 * 8 + (r & 7), tile = r >> 3;
        if (pair >= a.grp_pairs) return;
        const int prob = pair / a.grp_nsplit;
        split = pair - prob * a.grp_nsplit;
        tco = tile % a.tiles_co; tci = tile / a.tiles_co;
        u0 = (int)((long)split * a.grp_units / a.grp_nsplit);             // balanced, contiguous runs of units
        u1 = (int)((long)(split + 1) * a.grp_units / a.grp_nsplit);
        const TdrWg1GroupEntry e = static_cast<const TdrWg1GroupEntry*>(a.grp_tab)[prob];
        a.in = reinterpret_cast<const uint4*>(e.in); a.dout = reinterpret_cast<const uint4*>(e.dout);
        const bool direct = a.grp_nsplit == 1;                             // one slice: the workgroup's sums ARE the result
        a.part = direct ? e.g : e.part;
        dbout = direct ? e.db : e.dbpart;
    }
    const int co0 = tco * BMo, ci0 = tci * BNi;
    const long PS = (long)a.Hp * a.Wp;
    const int Gi = a.Cin >> 3, Go = a.Cout >> 3;
    const char* xbase = reinterpret_cast<const char*>(a.in);
    const char* dbase = reinterpret_cast<const char*>(a.dout);

    // ---- fragment addressing (see the header): lane = 16*g16 + nn; as a loader it points at pixel nn/4, channels 4*(nn%4)..
    const int nn = lane & 15, g16 = lane >> 4;
    const int jpx = nn >> 2, q = nn & 3, chalf = g16 & 1, kk = g16 >> 1;
    const int oct = chalf * 2 + (q >> 1);
    const int a_lane = ((wm * 4 + oct) * NS * 32 + 8 * kk + jpx) * 16 + (q & 1) * 8;     // + plane*32*16 + (16*ks + 4*r)*16
    const int b_lane = ((wn * 4 + oct) * NS * 34 + 8 * kk + jpx) * 16 + (q & 1) * 8;     // + plane*34*16 + (16*ks + 4*r + kx)*16

    f32x16 acc[9];
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[tp][r] = 0.f;
    f32x16 accb;
#pragma unroll
    for (int r = 0; r < 16; ++r) accb[r] = 0.f;
    const bool want_db = dbout != nullptr && tci == 0 && wn == 0;      // wave-uniform
    ws16x8 ones;
#pragma unroll
    for (int e = 0; e < 8; ++e) ones[e] = NS == 3 ? (short)0x3f80 : (short)0x3c00;      // 1.0 as bf16 / fp16

    for (int u = u0; u < u1; ++u) {      // (one unit unless GRP)
        const int chunk = u % a.chunks; const int t = u / a.chunks;
        const int strip = t % a.strips;
        const int n = t / a.strips;
        const int y0 = chunk * a.rc, y1 = min(y0 + a.rc, a.H);
        const int x0 = strip * 32;

        // ---- LDS-DMA sources: piece p of a row covers flat slots p*64 + lane of [octet][plane][column]; this wave issues pieces
        // wave, wave + 4, ..  The per-lane byte offsets (inside the image: 32 bits) are row-invariant; the image and row terms are
        // wave-uniform and ride in the scalar base of the load.
        constexpr int XPW = (XP + 3) / 4, DPW = (DP + 3) / 4;
        unsigned xoff[XPW], doff[DPW];
        const char* xb = xbase + (long)n * Gi * NS * PS * 16;
        const char* db = dbase + (long)n * Go * NS * PS * 16;
        bool dcol[DPW];
#pragma unroll
        for (int i = 0; i < XPW; ++i) {
            // input row piece: columns beyond the padded row are clamped to the right border (zero)
            const int f = min((wave + 4 * i) * 64 + lane, NOi * NS * 34 - 1);
            const int op = f / 34, c = f - op * 34;
            const int oc = min((ci0 >> 3) + (op / NS), Gi - 1);
            xoff[i] = (unsigned)((((long)oc * NS + (op % NS)) * PS + min(x0 + c, a.Wp - 1)) * 16);
        }
#pragma unroll
        for (int i = 0; i < DPW; ++i) {
            // gradient row piece: pixels outside the image must contribute ZERO: they are read from the (0, 0) border slot
            const int f = (wave + 4 * i) * 64 + lane;
            const int op = f >> 5, c = f & 31;
            const int oc = min((co0 >> 3) + (op / NS), Go - 1);
            dcol[i] = x0 + c < a.W;
            doff[i] = (unsigned)((((long)oc * NS + (op % NS)) * PS) * 16);
        }
        // LDS-DMA by inline asm: hipcc puts s_waitcnt vmcnt(0) in front of every LDS read that follows a __builtin LDS-DMA it
        // cannot prove disjoint (here: all of them), which would serialise the row loads with the MFMAs of the step.  Pieces
        // issued this way are invisible to its bookkeeping; they are waited for by the vmcnt(0) + barrier that ends every step.
        auto glds = [&](const char* base, unsigned off, uint4* dst) {      // base: wave-uniform
            const unsigned l = (unsigned)(uintptr_t)(__attribute__((address_space(3))) char*)dst;
            unsigned keep;
            asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %3\n\ts_mov_b32 m0, %0"
                         : "=&s"(keep) : "v"(off), "s"(l), "s"(base) : "memory");
        };
        auto issue_x_row = [&](int prow) {      // padded input row prow -> ring slot prow % XS
            uint4* dst = sX + (prow % XS) * XR;
            const long rowb = (long)min(prow, a.Hp - 1) * a.Wp * 16;
#pragma unroll
            for (int i = 0; i < XPW; ++i)
                if (wave + 4 * i < XP) glds(xb + rowb, xoff[i], dst + (wave + 4 * i) * 64);
        };
        auto issue_d_row = [&](int y) {
            uint4* dst = sD + (y % DS) * DR;
            const bool yok = y < a.H;
            const unsigned rowb = (unsigned)(((long)(y + 1) * a.Wp + x0 + 1) * 16);
#pragma unroll
            for (int i = 0; i < DPW; ++i)
                if (wave + 4 * i < DP) {
                    const int c = ((wave + 4 * i) * 64 + lane) & 31;
                    glds(db, doff[i] + ((yok && dcol[i]) ? rowb + c * 16 : 0u), dst + (wave + 4 * i) * 64);
                }
        };

        // ---- prologue: halo rows y0, y0+1 (+ the first step's new rows) and the first step's gradient rows
        issue_x_row(y0); issue_x_row(y0 + 1);
#pragma unroll
        for (int r = 0; r < RS; ++r) { issue_x_row(y0 + 2 + r); issue_d_row(y0 + r); }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");

        for (int y = y0; y < y1; y += RS) {
            // rows of the next step (clamped loads past the chunk are harmless: their ring slots are not read again)
#pragma unroll
            for (int r = 0; r < RS; ++r) { issue_x_row(y + RS + 2 + r); issue_d_row(y + RS + r); }
#pragma unroll
            for (int uu = 0; uu < 2 * RS / WK; ++uu) {
                const int ku = wk + uu * WK;                 // k-step of the step: row ku / 2, pixels 16 * (ku % 2) ..
                const int yr = y + (ku >> 1), ks = ku & 1;
                if (yr < y1) {
                    const char* pd = reinterpret_cast<const char*>(sD + (yr % DS) * DR) + a_lane + ks * 256;
                    ws16x8 ap[NS];                       // gradient planes h, m (, l)
#pragma unroll
                    for (int s = 0; s < NS; ++s) ap[s] = tr_frag(pd, s * 32 * 16, s * 32 * 16 + 64);
                    if (want_db) {
#pragma unroll
                        for (int s = NS - 1; s >= 0; --s) accb = wg_mfma<NS>(ap[s], ones, accb);
                    }
                    // small cross terms first, the dominant h*h last
                    constexpr int NPR = NS == 3 ? 6 : 3;
                    constexpr int PA[6] = {NS == 3 ? 2 : 1, 0, NS == 3 ? 1 : 0, 1, 0, 0};      // pair: mh hm hh ; triple: lh hl mm mh hm hh
                    constexpr int PB[6] = {0, NS == 3 ? 2 : 1, NS == 3 ? 1 : 0, 0, 1, 0};
#pragma unroll
                    for (int ky = 0; ky < 3; ++ky) {
                        const char* px = reinterpret_cast<const char*>(sX + ((yr + ky) % XS) * XR) + b_lane + ks * 256;
                        ws16x8 bp[NS][3];
#pragma unroll
                        for (int s = 0; s < NS; ++s)
#pragma unroll
                            for (int kx = 0; kx < 3; ++kx) bp[s][kx] = tr_frag(px, s * 34 * 16 + kx * 16, s * 34 * 16 + kx * 16 + 64);
#pragma unroll
                        for (int pr = 0; pr < NPR; ++pr)
#pragma unroll
                            for (int kx = 0; kx < 3; ++kx) acc[ky * 3 + kx] = wg_mfma<NS>(ap[PA[pr]], bp[PB[pr]][kx], acc[ky * 3 + kx]);
                    }
                }
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        }
    }

    // ---- waves that split K inside the block are summed through LDS in a fixed order (wk = 1, 2, ..)
    const int j = lane & 31, kg = lane >> 5;
    if constexpr (WK > 1) {
        float* red = reinterpret_cast<float*>(smem4);           // 10 x 16 x 64 floats = 40 KiB (the rings are free now)
#pragma unroll
        for (int w = 1; w < WK; ++w) {
            __syncthreads();
            if (wk == w) {
#pragma unroll
                for (int tp = 0; tp < 9; ++tp)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[(tp * 16 + r) * 64 + lane] = acc[tp][r];
#pragma unroll
                for (int r = 0; r < 16; ++r) red[(9 * 16 + r) * 64 + lane] = accb[r];
            }
            __syncthreads();
            if (wk == 0) {
#pragma unroll
                for (int tp = 0; tp < 9; ++tp)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[tp][r] += red[(tp * 16 + r) * 64 + lane];
#pragma unroll
                for (int r = 0; r < 16; ++r) accb[r] += red[(9 * 16 + r) * 64 + lane];
            }
        }
        if (wk != 0) return;
    }
    // partial[split][co][ci][tap]
    float* part = a.part + (long)split * a.Cout * a.Cin * 9;
    const int ci = ci0 + wn * 32 + j;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int co = co0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * kg;
        if (co < a.Cout && ci < a.Cin) {
#pragma unroll
            for (int tp = 0; tp < 9; ++tp) part[((long)co * a.Cin + ci) * 9 + tp] = acc[tp][r];
        }
        if (want_db && j == 0 && co < a.Cout) dbout[(long)split * a.Cout + co] = accb[r];
    }
}

// out[e] = sum_s part[s][e] in fixed order; blocks >= nb_main reduce the bias-gradient partials.  Block = 64 elements x KL
// partial-lanes, eight partials in flight per thread (as wgrad_reduce_kernel of tdr_wgrad_mfma.hip).
template <int KL>
__device__ __forceinline__ void wgp_reduce_block(const float* __restrict__ part, long elems, int nsplit, float* __restrict__ out, int nb_main,
                                                 const float* __restrict__ part2, long elems2, float* __restrict__ out2, int bx) {
    __shared__ float red[KL][64];
    const int lane = threadIdx.x & 63, kl = threadIdx.x >> 6;
    const bool second = bx >= nb_main;
    const float* pbase = second ? part2 : part;
    const long ne = second ? elems2 : elems;
    float* o = second ? out2 : out;
    const long e = (bx - (second ? nb_main : 0)) * 64L + lane;
    const float* p = pbase + (e < ne ? e : ne - 1);
    float s0 = 0.f;
    for (int k = kl; k < nsplit; k += 8 * KL) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = k + u * KL < nsplit ? p[(long)(k + u * KL) * ne] : 0.f;
        s0 += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
    red[kl][lane] = s0;
    __syncthreads();
    if (kl == 0 && e < ne) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < KL; ++q) t += red[q][lane];
        o[e] = t;
    }
}

template <int KL>
__global__ __launch_bounds__(64 * KL) void wgrad_p16_reduce_kernel(const float* __restrict__ part, long elems, int nsplit, float* __restrict__ out,
                                                                   int nb_main, const float* __restrict__ part2, long elems2, float* __restrict__ out2) {
    wgp_reduce_block<KL>(part, elems, nsplit, out, nb_main, part2, elems2, out2, (int)blockIdx.x);
}

// the same for every problem of a grouped launch (blockIdx.y = table row): a problem's sums depend on its own partials alone, in slice
// order 0 .. nsplit - 1 -- the same bits wherever its row sits in the table
template <int KL>
__global__ __launch_bounds__(64 * KL) void wgrad_p16_reduce_kernel_grp(const TdrWg1GroupEntry* __restrict__ tab, long elems, int nsplit, int Cout,
                                                                       int nb_main) {
    const TdrWg1GroupEntry e = tab[blockIdx.y];
    if ((int)blockIdx.x >= nb_main && (e.db == nullptr || e.dbpart == nullptr)) return;      // (block-uniform)
    wgp_reduce_block<KL>(e.part, elems, nsplit, e.g, nb_main, e.dbpart, (long)Cout, e.db, (int)blockIdx.x);
}

struct WgP16Plan { int cfg, bm, bn, strips, chunks, rc, nsplit; };

long wgp_want_total() {
    static const long want_total = tdr_tune_env("TDR_WGP_WANT") ? atol(tdr_tune_env("TDR_WGP_WANT")) : 512;
    return want_total;
}

// rows per chunk for `want` workgroups per output tile: never below 8 (the two halo rows of a chunk), whole steps, at most the image
WgP16Plan wgp_plan_for(const TdrWgradP16Desc* d, long want) {
    WgP16Plan p;
    p.cfg = (d->Cin <= 32 && d->Cout <= 32) ? 1 : 0;
    p.bm = p.cfg == 1 ? 32 : 64; p.bn = p.bm;
    const int rs = p.cfg == 1 ? 2 : 1;
    p.strips = tdr_cdiv(d->W, 32);
    if (want < 1) want = 1;
    const long rows = (long)d->N * p.strips * d->H;
    long rc = (rows + want - 1) / want;
    if (rc < 8) rc = 8;                                   // amortise the two halo rows of a chunk
    rc = (rc + rs - 1) / rs * rs;
    if (rc > d->H) rc = (d->H + rs - 1) / rs * rs;
    p.rc = (int)rc;
    p.chunks = tdr_cdiv(d->H, p.rc);
    p.nsplit = d->N * p.strips * p.chunks;
    return p;
}

// the kernel addresses inside one image of a plane tensor with 32-bit byte offsets
bool wgp_image_fits(const TdrWgradP16Desc* d) {
    const long c = d->Cin > d->Cout ? d->Cin : d->Cout;
    return c / 8 * 3 * (long)(d->H + 2) * (d->W + 2) * 16 < (1L << 32);
}

long wgp_out_tiles(const TdrWgradP16Desc* d) {
    const int t = (d->Cin <= 32 && d->Cout <= 32) ? 32 : 64;
    return (long)tdr_cdiv(d->Cout, t) * tdr_cdiv(d->Cin, t);
}

WgP16Plan wgp_plan(const TdrWgradP16Desc* d) { return wgp_plan_for(d, wgp_want_total() / wgp_out_tiles(d)); }

// grouped: the workgroups are shared by nprob problems.  units = the (n, strip, chunk) pieces of a problem's K at the chunk length that
// many slices want; nsplit = clamp(want_total / (nprob * out_tiles), 1, units) slices per problem, each a run of units / nsplit units
// (+ 1 for some: balanced)
struct WgP16GroupPlan { WgP16Plan p; int units, nsplit; };

WgP16GroupPlan wgp_group_plan(const TdrWgradP16Desc* d, int nprob) {
    WgP16GroupPlan gp;
    long want = wgp_want_total() / ((long)nprob * wgp_out_tiles(d));
    if (want < 1) want = 1;
    gp.p = wgp_plan_for(d, want);
    gp.units = gp.p.nsplit;
    gp.nsplit = (int)(want < gp.units ? want : gp.units);
    return gp;
}

template <int WM, int WN, int WK, int NS, bool GRP = false>
int launch_wgp(const WgP16Args& a, const WgP16Plan& p, const TdrWgradP16Desc* d, hipStream_t st) {
    constexpr int RS = WK == 4 ? 2 : 1, NOo = 4 * WM, NOi = 4 * WN;
    constexpr int XR = ((NOi * NS * 34 + 63) / 64) * 64, DR = NOo * NS * 32;
    size_t lds = (size_t)((2 * RS + 2) * XR + 2 * RS * DR) * 16;
    if (WK > 1 && lds < 10 * 16 * 64 * 4) lds = 10 * 16 * 64 * 4;
    dim3 grid(p.nsplit, tdr_cdiv(d->Cout, 32 * WM), tdr_cdiv(d->Cin, 32 * WN));
    if (GRP) grid = dim3((unsigned)tdr_cdiv(a.grp_pairs, 8) * 8 * a.tiles_co * a.tiles_ci);      // chunks of 8 pairs x T tiles
    auto kern = wgrad3x3_p16_kernel<WM, WN, WK, NS, GRP>;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        attr_set = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, a);
    TDR_LAUNCH_CHECK(GRP ? "wgrad3x3_p16_kernel<grouped>" : "wgrad3x3_p16_kernel");
    return TDR_OK;
}

}  // namespace

extern "C" int64_t tdr_wgrad3x3_p16_ws_floats(const TdrWgradP16Desc* d) {
    const WgP16Plan p = wgp_plan(d);
    return (int64_t)p.nsplit * d->Cout * d->Cin * 9 + (int64_t)p.nsplit * d->Cout;
}

extern "C" int tdr_wgrad3x3_p16(const TdrWgradP16Desc* d, void* stream) {
    TDR_REQUIRE(d && d->in16 && d->dout16 && d->g && d->ws, "tdr_wgrad3x3_p16: null pointer");
    TDR_REQUIRE(d->Cin % 16 == 0 && d->Cout % 16 == 0, "tdr_wgrad3x3_p16: channel counts must be multiples of 16 (%d, %d)", d->Cin, d->Cout);
    TDR_REQUIRE(wgp_image_fits(d), "tdr_wgrad3x3_p16: a plane image of more than 4 GiB");
    const WgP16Plan p = wgp_plan(d);
    const int64_t need = tdr_wgrad3x3_p16_ws_floats(d);
    TDR_REQUIRE(d->ws_floats >= need, "tdr_wgrad3x3_p16: workspace too small (%lld < %lld)", (long long)d->ws_floats, (long long)need);
    WgP16Args a;
    a.in = (const uint4*)d->in16; a.dout = (const uint4*)d->dout16;
    a.Cin = d->Cin; a.Cout = d->Cout; a.H = d->H; a.W = d->W; a.Hp = d->H + 2; a.Wp = d->W + 2;
    a.strips = p.strips; a.chunks = p.chunks; a.rc = p.rc;
    a.part = d->ws;
    a.grp_tab = nullptr; a.grp_pairs = a.grp_nsplit = a.grp_units = a.tiles_co = a.tiles_ci = 0;
    a.dbpart = d->db ? d->ws + (int64_t)p.nsplit * d->Cout * d->Cin * 9 : nullptr;
    hipStream_t st = (hipStream_t)stream;
    TDR_REQUIRE(d->fmt == 0 || d->fmt == 1 || d->fmt == 2, "tdr_wgrad3x3_p16: plane format %d (1: bf16 triple, 2: fp16 pair)", d->fmt);
    int rc;
    if (d->fmt == 1) rc = p.cfg == 1 ? launch_wgp<1, 1, 4, 3>(a, p, d, st) : launch_wgp<2, 2, 1, 3>(a, p, d, st);
    else rc = p.cfg == 1 ? launch_wgp<1, 1, 4, 2>(a, p, d, st) : launch_wgp<2, 2, 1, 2>(a, p, d, st);
    if (rc != TDR_OK) return rc;
    const long elems = (long)d->Cout * d->Cin * 9;
    const int nb_main = tdr_cdiv(elems, 64), nb2 = d->db ? tdr_cdiv(d->Cout, 64) : 0;
    if (p.nsplit <= 8)
        hipLaunchKernelGGL(wgrad_p16_reduce_kernel<1>, dim3(nb_main + nb2), dim3(64), 0, st, d->ws, elems, p.nsplit, d->g, nb_main, a.dbpart,
                           (long)d->Cout, d->db);
    else if (p.nsplit <= 64)
        hipLaunchKernelGGL(wgrad_p16_reduce_kernel<4>, dim3(nb_main + nb2), dim3(256), 0, st, d->ws, elems, p.nsplit, d->g, nb_main, a.dbpart,
                           (long)d->Cout, d->db);
    else
        hipLaunchKernelGGL(wgrad_p16_reduce_kernel<16>, dim3(nb_main + nb2), dim3(1024), 0, st, d->ws, elems, p.nsplit, d->g, nb_main, a.dbpart,
                           (long)d->Cout, d->db);
    TDR_LAUNCH_CHECK("wgrad_p16_reduce_kernel");
    return TDR_OK;
}

// ---- grouped form: nprob problems of ONE shape and plane format in one launch (+ one table-driven reduction unless nsplit == 1).
// floats of workspace PER PROBLEM: [nsplit][Cout][Cin][9] partials, then [nsplit][Cout] bias-gradient partials; 0 with one slice
extern "C" int64_t tdr_wgrad3x3_p16_group_ws_floats(const TdrWgradP16Desc* d, int nprob) {
    if (!d || nprob < 1) return 0;
    const WgP16GroupPlan gp = wgp_group_plan(d, nprob);
    if (gp.nsplit == 1) return 0;
    return (int64_t)gp.nsplit * d->Cout * d->Cin * 9 + (int64_t)gp.nsplit * d->Cout;
}

// the plan a group gets: slices per problem, units per problem, the most units one workgroup walks (cdiv(units, nsplit))
extern "C" int tdr_wgrad3x3_p16_group_plan(const TdrWgradP16Desc* d, int nprob, int* nsplit, int* units, int* units_per_wg) {
    TDR_REQUIRE(d && nprob > 0, "tdr_wgrad3x3_p16_group_plan: null argument");
    const WgP16GroupPlan gp = wgp_group_plan(d, nprob);
    if (nsplit) *nsplit = gp.nsplit;
    if (units) *units = gp.units;
    if (units_per_wg) *units_per_wg = tdr_cdiv(gp.units, gp.nsplit);
    return TDR_OK;
}

// d: the common shape and format (N, Cin, Cout, H, W, fmt); its pointers are ignored.  table: TdrWg1GroupEntry[nprob] in DEVICE memory
// (in = in16, dout = dout16, part = the problem's workspace, dbpart = part + nsplit * Cout * Cin * 9 or NULL, g, db or NULL; part and
// dbpart are not read when tdr_wgrad3x3_p16_group_ws_floats is 0).
extern "C" int tdr_wgrad3x3_p16_group(const TdrWgradP16Desc* d, int nprob, const void* table, void* stream) {
    TDR_REQUIRE(d && table && nprob > 0, "tdr_wgrad3x3_p16_group: null argument");
    TDR_REQUIRE(d->Cin % 16 == 0 && d->Cout % 16 == 0, "tdr_wgrad3x3_p16_group: channel counts must be multiples of 16 (%d, %d)", d->Cin, d->Cout);
    TDR_REQUIRE(d->fmt == 0 || d->fmt == 1 || d->fmt == 2, "tdr_wgrad3x3_p16_group: plane format %d (1: bf16 triple, 2: fp16 pair)", d->fmt);
    TDR_REQUIRE(wgp_image_fits(d), "tdr_wgrad3x3_p16_group: a plane image of more than 4 GiB");
    const WgP16GroupPlan gp = wgp_group_plan(d, nprob);
    const WgP16Plan& p = gp.p;
    WgP16Args a;
    a.in = nullptr; a.dout = nullptr; a.part = nullptr; a.dbpart = nullptr;
    a.Cin = d->Cin; a.Cout = d->Cout; a.H = d->H; a.W = d->W; a.Hp = d->H + 2; a.Wp = d->W + 2;
    a.strips = p.strips; a.chunks = p.chunks; a.rc = p.rc;
    a.grp_tab = table; a.grp_nsplit = gp.nsplit; a.grp_units = gp.units;
    a.tiles_co = tdr_cdiv(d->Cout, p.bm); a.tiles_ci = tdr_cdiv(d->Cin, p.bn);
    const long pairs = (long)nprob * gp.nsplit;
    TDR_REQUIRE(pairs * a.tiles_co * a.tiles_ci < (1L << 30), "tdr_wgrad3x3_p16_group: too many workgroups (%ld pairs)", pairs);
    a.grp_pairs = (int)pairs;
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (d->fmt == 1) rc = p.cfg == 1 ? launch_wgp<1, 1, 4, 3, true>(a, p, d, st) : launch_wgp<2, 2, 1, 3, true>(a, p, d, st);
    else rc = p.cfg == 1 ? launch_wgp<1, 1, 4, 2, true>(a, p, d, st) : launch_wgp<2, 2, 1, 2, true>(a, p, d, st);
    if (rc != TDR_OK || gp.nsplit == 1) return rc;
    const long elems = (long)d->Cout * d->Cin * 9;
    const int nb_main = tdr_cdiv(elems, 64), nb2 = tdr_cdiv(d->Cout, 64);
    const TdrWg1GroupEntry* tab = static_cast<const TdrWg1GroupEntry*>(table);
    if (gp.nsplit <= 8)
        hipLaunchKernelGGL(wgrad_p16_reduce_kernel_grp<1>, dim3(nb_main + nb2, nprob), dim3(64), 0, st, tab, elems, gp.nsplit, d->Cout, nb_main);
    else if (gp.nsplit <= 64)
        hipLaunchKernelGGL(wgrad_p16_reduce_kernel_grp<4>, dim3(nb_main + nb2, nprob), dim3(256), 0, st, tab, elems, gp.nsplit, d->Cout, nb_main);
    else
        hipLaunchKernelGGL(wgrad_p16_reduce_kernel_grp<16>, dim3(nb_main + nb2, nprob), dim3(1024), 0, st, tab, elems, gp.nsplit, d->Cout, nb_main);
    TDR_LAUNCH_CHECK("wgrad_p16_reduce_kernel_grp");
    return TDR_OK;
}
