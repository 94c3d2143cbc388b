// Fused NAFBlock chains, the training entry points: tdr_naf_tail_fwd / tdr_naf_head_fwd (the KEEP = true instantiations of the forward
// kernels, every tensor the backward pass reads is written) and tdr_naf_tail_bwd / tdr_naf_head_bwd (the data-gradient chains).  The
// kernels and the forward launchers are tdr_nafblock_chain.h; this unit's object holds the training kernels and nothing else.
#include "tdr_nafblock_chain.h"

#ifdef TDR_NB_PROBE
extern "C" int tdr_nb_probe_read(unsigned long long* host) {
    return hipMemcpyFromSymbol(host, HIP_SYMBOL(nb_probe_buf), sizeof(unsigned long long) * 64) == hipSuccess ? 0 : -1;
}
#endif

extern "C" int tdr_naf_tail_supported(int C, int HW) { return naf_chain_supported(C, HW) ? 1 : 0; }
extern "C" int tdr_naf_tail_fwd(const TdrNafTailDesc* d, void* stream) { return naf_tail_fwd_launch<true>(d, stream); }
extern "C" int tdr_naf_head_fwd(const TdrNafHeadFwdDesc* d, void* stream) { return naf_head_fwd_launch<true>(d, stream); }

extern "C" int64_t tdr_naf_tail_bwd_ws_floats(int N, int C, int HW) {
    const int nparts = N * (HW / NPX);
    return (int64_t)nparts * 2 * C + tdr_pair_sum_mid_floats(nparts, C);
}

extern "C" int tdr_naf_tail_bwd(const TdrNafTailBwdDesc* d, void* stream) {
    TDR_REQUIRE(d && d->dout && d->gamma && d->t4 && d->y && d->mu && d->rs && d->lnw && d->w5t && d->w4t && d->dt4 && d->dy && d->ws,
                "tdr_naf_tail_bwd: null pointer");
    TDR_REQUIRE((d->gw != nullptr) == (d->gb != nullptr), "tdr_naf_tail_bwd: gw and gb are given together or not at all");
    TDR_REQUIRE(tdr_naf_tail_supported(d->C, d->HW), "tdr_naf_tail_bwd: needs C in {32, 64, 128, 256} and HW %% 64 == 0 (got C=%d HW=%d)", d->C, d->HW);
    TDR_REQUIRE(d->w_fmt == 2 || d->w_fmt == 1, "tdr_naf_tail_bwd: weights must be packed with tdr_pack_weights_hx2 / _bx3 (mode DGRAD_S1)");
    TDR_REQUIRE(d->dout_ns % 4 == 0 && (reinterpret_cast<uintptr_t>(d->dout) & 15) == 0, "tdr_naf_tail_bwd: dout must be 16-byte aligned");
    TailBwdArgs a;
    a.dout = d->dout; a.dout_ns = d->dout_ns; a.gamma = d->gamma; a.t4 = d->t4; a.t4_ns = d->t4_ns; a.y = d->y; a.y_ns = d->y_ns;
    a.mu = d->mu; a.rs = d->rs; a.lnw = d->lnw;
    a.w5t = reinterpret_cast<const uint4*>(d->w5t); a.w4t = reinterpret_cast<const uint4*>(d->w4t);
    a.dt4 = d->dt4; a.dt4_ns = d->dt4_ns; a.dy = d->dy; a.dy_ns = d->dy_ns; a.part = d->ws; a.HW = d->HW;
    a.res = d->dout; a.res_ns = d->dout_ns;
    a.c_out = d->c_out > 0 ? d->c_out : d->C;
    TDR_REQUIRE(a.c_out == d->C || (a.c_out * 2 == d->C && a.c_out % 32 == 0), "tdr_naf_tail_bwd: c_out must be C or C / 2 (a multiple of 32)");
    a.w3t = reinterpret_cast<const uint4*>(d->w3t); a.beta = d->beta; a.sca = d->sca; a.dgp = d->dgp; a.dgp_ns = d->dgp_ns;
    TDR_REQUIRE(!d->w3t || (d->beta && d->sca && d->dgp), "tdr_naf_tail_bwd: the conv3 stage needs beta, sca and dgp");
    const bool bx = d->w_fmt == 1;
    NAF_DISPATCH_CS(naf_tail_bwd_kernel, NAF_COMMA false, , naf_bwd_lds_bytes(d->C, bx), a, d, stream);
    TDR_LAUNCH_CHECK("naf_tail_bwd_kernel");
    if (!d->gw) return TDR_OK;            // the caller finishes the LayerNorm parameter gradients itself (tdr_pair_sum_partials on ws)
    return tdr_pair_sum_partials(d->ws, d->N * (d->HW / NPX), d->C, d->gw, d->gb, d->ws + (long)d->N * (d->HW / NPX) * 2 * d->C, stream);
}

extern "C" int tdr_naf_head_bwd(const TdrNafHeadBwdDesc* d, void* stream) {
    TDR_REQUIRE(d && d->dt1 && d->x && d->mu && d->rs && d->lnw && d->w1t && d->res && d->dx && d->ws, "tdr_naf_head_bwd: null pointer");
    TDR_REQUIRE((d->gw != nullptr) == (d->gb != nullptr), "tdr_naf_head_bwd: gw and gb are given together or not at all");
    TDR_REQUIRE(tdr_naf_tail_supported(d->C, d->HW), "tdr_naf_head_bwd: needs C in {32, 64, 128, 256} and HW %% 64 == 0 (got C=%d HW=%d)", d->C, d->HW);
    TDR_REQUIRE(d->w_fmt == 2 || d->w_fmt == 1, "tdr_naf_head_bwd: weights must be packed with tdr_pack_weights_hx2 / _bx3 (mode DGRAD_S1)");
    TDR_REQUIRE(d->dt1_ns % 4 == 0 && (reinterpret_cast<uintptr_t>(d->dt1) & 15) == 0, "tdr_naf_head_bwd: dt1 must be 16-byte aligned");
    TailBwdArgs a;
    a.dout = d->dt1; a.dout_ns = d->dt1_ns; a.gamma = nullptr; a.t4 = nullptr; a.t4_ns = 0; a.y = d->x; a.y_ns = d->x_ns;
    a.mu = d->mu; a.rs = d->rs; a.lnw = d->lnw;
    a.w5t = nullptr; a.w4t = reinterpret_cast<const uint4*>(d->w1t);
    a.dt4 = nullptr; a.dt4_ns = 0; a.res = d->res; a.res_ns = d->res_ns; a.dy = d->dx; a.dy_ns = d->dx_ns; a.part = d->ws; a.HW = d->HW;
    a.c_out = d->C;
    a.w3t = nullptr; a.beta = nullptr; a.sca = nullptr; a.dgp = nullptr; a.dgp_ns = 0;
    const bool bx = d->w_fmt == 1;
    NAF_DISPATCH_CS(naf_tail_bwd_kernel, NAF_COMMA true, , naf_bwd_lds_bytes(d->C, bx), a, d, stream);
    TDR_LAUNCH_CHECK("naf_head_bwd_kernel");
    if (!d->gw) return TDR_OK;
    return tdr_pair_sum_partials(d->ws, d->N * (d->HW / NPX), d->C, d->gw, d->gb, d->ws + (long)d->N * (d->HW / NPX) * 2 * d->C, stream);
}
