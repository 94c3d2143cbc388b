"""Float64 references, seeded input builders and bars for the streaming kernels of csrc/tdr_pointwise.hip (LayerNorm2d, the SCA
chain, the partial-sum finishers, channel_sum, the row copies) and the depthwise-gate forward stencils of csrc/tdr_dwsg.hip.  Torch on
the CPU only; nothing here imports the GPU package.  tests/test_stream_reference.py pins this module on the host,
tests/test_hip_stream_float64.py holds the kernels to it.

Every reference takes a dtype: run in float64 on the float32 inputs cast up it is the truth, run in float32 it is the yardstick --
e32 = max |f32 run - f64 run| is what float32 arithmetic leaves in the reference itself.  Bars (none is typed in):
    element-wise outputs        _masa_ref.bar(e32, ref64) = max(8 e32, 4 float32 ulp of max |ref64|)
    outputs summed over pixels  the larger of that and sum_bar(depth, terms) = depth 2^-24 max_c sum_i |t_i|, the worst-case error of
    or partial rows             ANY float32 summation of the float64 terms t_i whose longest path has `depth` additions; the *_depth
                                functions below count that path in the kernel's own loops
    pure sums and moves         also run on integer-valued inputs (|x| <= 8: every partial sum is exact in float32 in any order) and
                                held to equality with the float64 result
The planted defects (ln_ref(defect=...), dropping a partial row) are what test_stream_reference.py uses to show that each bar can fail."""
import math

import torch
import torch.nn.functional as F

from _masa_ref import bar, case_seed, maxabs

U32 = 2.0 ** -24          # unit roundoff of float32: one addition adds at most U32 * |partial sum|
EPS = 1e-6
PAD_LO, PAD_HI = 4, 3     # channels around a channel slice of a wider tensor


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def cdiv(a, b):
    return -(-a // b)


def sum_bar(depth, abs_terms):
    """abs_terms: per output element sum_i |t_i| in float64"""
    return depth * U32 * abs_terms.double().max().item()


def reduced_bar(e32, ref64, depth, abs_terms):
    return max(bar(e32, ref64), sum_bar(depth, abs_terms))


def int_values(shape, g, lim=8):
    """integer-valued float32 in [-lim, lim]"""
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


# ------------------------------------------------------------------------------------------- reduction depths (float additions)
def fin_depth(nparts):
    """pair_sum_partials_kernel<16>: the thread's chain over every 32nd row (k += 2 KL), s0 + s1, the 16 LDS slices in order"""
    return cdiv(nparts, 32) + 1 + 16


def fold_depth(C2):
    """pair_fold_partials_kernel: a thread's slice of per = 256 / SL rows in four chains (per / 4 trips), (s0 + s1) + (s2 + s3), then
    the SL slice sums in order"""
    SL = 1 if C2 >= 256 else 256 // C2
    return cdiv(256 // SL, 4) + 2 + (SL if SL > 1 else 0)


def pair_sum_depth(nparts, C):
    if nparts > 1024:
        return fold_depth(2 * C) + fin_depth(cdiv(nparts, 256))
    return fin_depth(nparts)


def ln_tiles(N, HW):
    return N * cdiv(HW, 64)


def ln_bwd_depth(C, N, HW):
    """gw / gb of tdr_layernorm2d_bwd.
    C <= 128 (ln_bwd_kernel): per-thread trips of the persistent grid (ceil(tiles / grid) additions into aw / ab), the 6 wave steps,
                              the finisher over `grid` rows
    tiles <= 1024 (cached / generic<true>): the 6 wave steps over a tile's 64 pixels, the finisher over `tiles` rows
    else (ln_param_grad_kernel): per-thread trips over N HW / (16 splits x 256 threads), the 6 wave steps, the 3 additions over the
                              block's 4 waves, the finisher over 16 rows"""
    tiles = ln_tiles(N, HW)
    if C <= 128:
        grid = min(tiles, 256)
        return cdiv(tiles, grid) + 6 + fin_depth(grid)
    if tiles <= 1024:
        return 6 + fin_depth(tiles)
    return cdiv(N * HW, 16 * 256) + 6 + 3 + fin_depth(16)


def chansum_depth(N, HW):
    """chansum_kernel: per-thread trips over N HW / (32 splits x 256 threads), the 6 wave steps, (r0 + r1) + (r2 + r3), then
    chansum_finish_kernel's chain over the 32 splits"""
    return cdiv(N * HW, 32 * 256) + 6 + 2 + 32


def dw_geom(H, W):
    """launch geometry of the forward stencils (dw_geom of csrc/tdr_dw_stencil.h): rows per thread, column blocks, blocks per plane"""
    groups, lg = W // 4, 0
    while (1 << lg) < groups and lg < 8:
        lg += 1
    spb = 256 >> lg
    ncb = cdiv(groups, 1 << lg)
    rpt = max(1, min(8, cdiv(H, spb)))
    return rpt, ncb, ncb * cdiv(H, spb * rpt)


def pooled_depth(H, W):
    """dwsg_fwd's pool: per row of a thread's strip (o0 + o1) + (o2 + o3) and the addition into acc (3 rpt), the 6 wave steps,
    (r0 + r1) + (r2 + r3), dw_pool_finish_kernel's chain over the nb blocks of the plane, the rounding of the 1 / HW product"""
    rpt, _, nb = dw_geom(H, W)
    return 3 * rpt + 6 + 2 + (nb if nb > 1 else 0) + 1


# ---------------------------------------------------------------------------------------------------------------- LayerNorm2d
LN_DEFECTS = ('drop_pixel', 'short_stats', 'add_wide', 'uncentred_gw')


def ln_ref(x, w, b, go, add, add_C, center, dtype, defect=None):
    """x, go [N, C, H, W]; w [C]; b [C] or None; add [N, >= add_C, H, W] or None (added to the first add_C channels of gx).
    center = 0 is BiasFree_LayerNorm: y = x rstd w, the variance still taken about the mean, mu still returned.
    Returns dict(y, mu [N, HW], rstd [N, HW], gx, gw, gb, gw_abs, gb_abs) -- the *_abs are sum |t_i| of the terms of gw / gb.
    defect: one structural mistake of a kernel, for the host tier --
        drop_pixel    the last pixel of the last image is left out of gw / gb
        short_stats   the last channel is left out of the sums of the mean and the variance
        add_wide      add is applied to add_C + 1 channels
        uncentred_gw  x rstd in place of (x - mu) rstd in gw (wrong where center = 1)"""
    x, w = x.to(dtype), w.to(dtype)
    N, C = x.shape[:2]
    k = C - 1 if defect == 'short_stats' else C
    mu = x[:, :k].sum(1, keepdim=True) / C
    xc = x - mu
    var = (xc[:, :k] * xc[:, :k]).sum(1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(var + EPS)
    yh = xc * rstd
    yu = yh if center else x * rstd
    wv = w.view(1, -1, 1, 1)
    y = yu * wv
    if b is not None:
        y = y + b.to(dtype).view(1, -1, 1, 1)
    fwd = dict(y=y, mu=mu.reshape(N, -1), rstd=rstd.reshape(N, -1))
    if go is None:
        return fwd
    go = go.to(dtype)
    g = go * wv
    gx = g - yh * (g * yu).mean(1, keepdim=True)
    if center:
        gx = gx - g.mean(1, keepdim=True)
    gx = gx * rstd
    if add is not None:
        ka = add_C + (1 if defect == 'add_wide' else 0)
        gx[:, :ka] += add[:, :ka].to(dtype)
    t = go * (x * rstd if defect == 'uncentred_gw' else yu)
    gw, gb = t.sum((0, 2, 3)), go.sum((0, 2, 3))
    if defect == 'drop_pixel':
        gw = gw - t[-1, :, -1, -1]
        gb = gb - go[-1, :, -1, -1]
    return dict(fwd, gx=gx, gw=gw, gb=gb, gw_abs=t.abs().sum((0, 2, 3)), gb_abs=go.abs().sum((0, 2, 3)))


# forward dispatch table: (C, N, HW, center, regime, x is a channel slice)
LN_FWD_CASES = [
    (5, 2, 1, 1, 'randn', 0), (5, 2, 90, 0, 'offset', 1), (32, 1, 1, 0, 'randn', 0), (32, 2, 90, 1, 'dead', 0),          # ln_fwd_kernel<4,8>
    (33, 2, 63, 1, 'offset', 0), (64, 2, 90, 0, 'randn', 1),                                                             # <4,16>
    (65, 2, 64, 0, 'randn', 0), (128, 2, 65, 1, 'offset', 1),                                                            # <4,32>
    (129, 2, 65, 1, 'randn', 1), (256, 2, 63, 0, 'offset', 0),                                                           # <8,32>
    (257, 2, 64, 0, 'offset', 0), (512, 2, 63, 1, 'randn', 1), (512, 1, 65, 0, 'dead', 1),                               # <16,32>
    (513, 2, 77, 1, 'offset', 1), (513, 1, 257, 0, 'randn', 1), (768, 2, 77, 1, 'dead', 0), (768, 1, 257, 0, 'randn', 0),  # narrow<12>
    (769, 1, 257, 1, 'randn', 0), (1280, 1, 257, 0, 'offset', 1), (1536, 2, 257, 1, 'randn', 1),                         # narrow<24>
    (1537, 2, 70, 1, 'offset', 1), (1537, 1, 70, 0, 'randn', 1),                                                         # generic, C > 1536
    (513, 2, 16321, 1, 'randn', 0),          # generic: N ceil(HW / 64) = 512 exactly
    (513, 1, 64 * 511 - 5, 0, 'randn', 0),   # narrow<12>: N ceil(HW / 64) = 511, the other side of that boundary
]

# backward dispatch table: (C, N, HW, center, regime, add in none / full / part, x is a channel slice, add is a channel slice)
LN_BWD_CASES = [
    (5, 1, 1, 1, 'randn', 'full', 0, 1), (32, 2, 90, 1, 'randn', 'none', 0, 0),                   # ln_bwd_kernel<4,8>, one trip
    (32, 3, 6417, 0, 'offset', 'part', 1, 0), (32, 2, 65, 0, 'dead', 'full', 0, 0),               #   303 tiles on 256 blocks | dead pixels
    (33, 1, 65, 1, 'dead', 'part', 1, 0), (64, 2, 63, 0, 'randn', 'full', 1, 0),                  # ln_bwd_kernel<4,16>
    (64, 3, 6417, 1, 'offset', 'none', 0, 0),                                                     #   303 tiles
    (65, 2, 90, 0, 'randn', 'none', 0, 0), (128, 2, 65, 1, 'offset', 'part', 0, 1),               # ln_bwd_kernel<8,16>
    (128, 3, 6417, 0, 'randn', 'full', 1, 0), (128, 2, 63, 1, 'dead', 'none', 0, 0),              #   303 tiles | dead pixels
    (129, 2, 90, 1, 'randn', 'part', 1, 0), (256, 1, 63, 0, 'offset', 'full', 0, 0),              # ln_bwd_cached_kernel<16>
    (256, 2, 65, 1, 'dead', 'none', 0, 0),
    (257, 2, 65, 0, 'randn', 'none', 1, 0), (512, 2, 90, 1, 'offset', 'part', 0, 1),              # ln_bwd_cached_kernel<32>
    (512, 1, 64, 0, 'dead', 'full', 1, 0),
    (513, 2, 63, 1, 'randn', 'full', 1, 0), (1024, 1, 90, 0, 'offset', 'part', 1, 0),             # ln_bwd_generic_kernel<true>
    (1024, 2, 65, 1, 'dead', 'none', 0, 0),
    (129, 3, 148 * 148, 1, 'randn', 'part', 0, 0),                                                # ln_bwd_generic_kernel<false> +
    (129, 3, 148 * 148, 0, 'offset', 'none', 1, 0),                                               #   ln_param_grad_kernel: 1029 tiles,
    (129, 3, 148 * 148, 0, 'randn', 'full', 0, 1),                                                #   the last one of an image ragged
]
# one case per backward kernel template (the multi-trip ones of ln_bwd_kernel) for the exact gb run on integer-valued go
LN_BWD_EXACT_GB = [LN_BWD_CASES[i] for i in (2, 6, 9, 11, 15, 18, 20)]


def ln_fwd_kernel_name(C, N, HW):
    if C <= 512:
        return 'ln_fwd_kernel<%d,%d>' % ((4, 8) if C <= 32 else (4, 16) if C <= 64 else (4, 32) if C <= 128 else (8, 32) if C <= 256 else (16, 32))
    if C <= 1536 and ln_tiles(N, HW) < 512:
        return 'ln_fwd_narrow_kernel<%d>' % (12 if C <= 768 else 24)
    return 'ln_fwd_generic_kernel'


def ln_bwd_kernel_name(C, N, HW):
    if C <= 128:
        return 'ln_bwd_kernel<%d,%d>' % ((4, 8) if C <= 32 else (4, 16) if C <= 64 else (8, 16))
    if ln_tiles(N, HW) <= 1024:
        return 'ln_bwd_cached_kernel<%d>' % (16 if C <= 256 else 32) if C <= 512 else 'ln_bwd_generic_kernel<true>'
    return 'ln_bwd_generic_kernel<false>+ln_param_grad_kernel'


DEAD_VALUES = (0.5, 0.0)      # dyadic: C * 0.5 and (C * 0.5) / C are exact in float32 for every C of the tables


def dead_pixels(N, HW):
    """(image, pixel, value): two zero-variance pixels, neither the last pixel of the last image (the one drop_pixel leaves out)"""
    return [(0, 0, DEAD_VALUES[0]), (N - 1, HW // 2, DEAD_VALUES[1])]


def ln_x(C, N, HW, regime, g):
    """randn:  standard normal.
    offset: every seventh channel scaled by 8, then a per-pixel offset of +-50 standard deviations (over the channels of that pixel).
    dead:   randn with the pixels of dead_pixels() set to a constant over C."""
    x = torch.randn(N, C, 1, HW, generator=g)
    if regime == 'offset':
        x[:, ::7] *= 8.0
        sig = x.std(1, unbiased=False, keepdim=True)
        sign = torch.randint(0, 2, (N, 1, 1, HW), generator=g).float() * 2 - 1
        x = x + 50.0 * sig * sign
    elif regime == 'dead':
        for n, p, v in dead_pixels(N, HW):
            x[n, :, 0, p] = v
    else:
        assert regime == 'randn', regime
    return x


def ln_inputs(C, N, HW, center, regime, add='none', xs=0, as_=0, backward=True):
    """O(1) inputs of one LayerNorm case (backward=False: go is None, the reference stops after the forward).
    go is 4 at the last pixel of the last image, so that leaving that pixel out of gw / gb is visible whatever the seed.
    add: [N, add_C (+ padding), 1, HW]; 'part' -> add_C = max(1, C // 2) and the tensor handed to the kernel is a channel slice of
    `add_wide` (O(1) values all over: applying it to one channel too many reads the next one)."""
    g = _gen(case_seed('ln', C, N, HW, center, regime, add, xs, as_))
    x = ln_x(C, N, HW, regime, g)
    w = torch.randn(C, generator=g) * 0.3 + 1
    b = torch.randn(C, generator=g) * 0.2 if center else None
    go = None
    if backward:
        go = torch.randn(N, C, 1, HW, generator=g)
        go[-1, :, 0, -1] = 4.0
    inp = dict(C=C, N=N, HW=HW, center=center, regime=regime, x=x, w=w, b=b, go=go, xs=xs, add_wide=None, add_C=0, add_lo=0,
               dead=dead_pixels(N, HW) if regime == 'dead' else [])
    if add != 'none':
        add_C = C if add == 'full' else max(1, C // 2)
        lo = PAD_LO if as_ else 0
        hi = 0 if (add == 'full' and not as_) else PAD_HI
        inp.update(add_wide=torch.randn(N, lo + add_C + hi, 1, HW, generator=g), add_C=add_C, add_lo=lo)
    return inp


def ln_add(inp):
    """the add operand as the kernel and the reference see it from channel 0 on (the padding after add_C included)"""
    return None if inp['add_wide'] is None else inp['add_wide'][:, inp['add_lo']:]


def live_mask(inp):
    """[N, HW] float mask: 0 at the dead pixels"""
    m = torch.ones(inp['N'], inp['HW'], dtype=torch.float64)
    for n, p, _ in inp['dead']:
        m[n, p] = 0
    return m


def masked(t, m):
    """t [N, C, 1, HW] or [N, HW] times the pixel mask m [N, HW]"""
    return t.double() * (m.view(m.shape[0], 1, 1, -1) if t.dim() == 4 else m)


LN_FORWARD = ('y', 'mu', 'rstd')
LN_ELEMENTWISE = LN_FORWARD + ('gx',)


def ln_reference(inp, defect=None):
    """float64 reference and the bars of one case: r[k] the float64 outputs; r['bar'][k], r['e32'][k] for y, mu, rstd, gx over the live
    pixels, for gw, gb with the summation bound; r['bar_dead'][k], r['e32_dead'][k] over the dead pixels alone (their rstd = 1 / sqrt(eps)
    would otherwise set the bar of every other pixel).  With a defect: only the float64 outputs of the defective reference."""
    args = (inp['x'], inp['w'], inp['b'], inp['go'], ln_add(inp), inp['add_C'], inp['center'])
    if defect is not None:
        return ln_ref(*args, torch.float64, defect)
    r, r32 = ln_ref(*args, torch.float64), ln_ref(*args, torch.float32)
    m = live_mask(inp)
    r.update(e32={}, bar={}, e32_dead={}, bar_dead={}, live=m)
    for k in LN_ELEMENTWISE if inp['go'] is not None else LN_FORWARD:
        r['e32'][k] = maxabs(masked(r32[k], m), masked(r[k], m))
        r['bar'][k] = bar(r['e32'][k], masked(r[k], m))
        if inp['dead']:
            r['e32_dead'][k] = maxabs(masked(r32[k], 1 - m), masked(r[k], 1 - m))
            r['bar_dead'][k] = bar(r['e32_dead'][k], masked(r[k], 1 - m))
    if inp['go'] is None:
        return r
    depth = ln_bwd_depth(inp['C'], inp['N'], inp['HW'])
    for k in ('gw', 'gb'):
        r['e32'][k] = maxabs(r32[k], r[k])
        r['bar'][k] = reduced_bar(r['e32'][k], r[k], depth, r[k + '_abs'])
    return r


# ------------------------------------------------------------------------------------------------------------------ SCA chain
SCA_C, SCA_N = (6, 32, 70, 256, 320, 512), (1, 3)
SCA_CASES = [(C, N, 'random') for C in SCA_C for N in SCA_N] + [(C, 3, 'integer') for C in SCA_C]
PARAM_CASES = [(32, 32, 0), (6, 300, 3), (70, 520, 0)]          # (Cout, Cin, extra rows of w / b / gamma beyond Cout)
SCA_OUT = ('s', 'dw3', 'db3', 'dbeta', 'dwsca', 'dbsca', 'dpooled')
SCA_HW = 2                    # 2 x 2 maps: pooled, G3 and S3 of the dyadic g / dy below are exact in float32


def sca_ref(g, dy, w3, b3, beta, wsca, bsca, dtype):
    """as tests/test_hip_kernels.py::test_sca_and_param_chains writes it: autograd through conv2d(pooled) -> conv2d(g * s) * beta.
    g, dy [N, C, H, W]; returns dict(s [N, C], dw3, db3, dbeta, dwsca, dbsca, dpooled)"""
    N, C = g.shape[:2]
    g, dy = g.to(dtype), dy.to(dtype)
    w3, b3, beta, wsca, bsca = (t.to(dtype).clone().requires_grad_(True) for t in (w3, b3, beta, wsca, bsca))
    pooled = g.mean(dim=(2, 3)).requires_grad_(True)
    s = F.conv2d(pooled.view(N, C, 1, 1), wsca.view(C, C, 1, 1), bsca)
    out = F.conv2d(g * s, w3.view(C, C, 1, 1), b3) * beta.view(1, C, 1, 1)
    out.backward(dy)
    return dict(s=s.detach().view(N, C), dw3=w3.grad, db3=b3.grad, dbeta=beta.grad, dwsca=wsca.grad, dbsca=bsca.grad, dpooled=pooled.grad)


def param_ref(g, dy, w, b, gamma, dtype):
    """the gamma chain of scaled_conv_param_grads: autograd through conv2d(g, w, b) * gamma.  g [N, Cin, H, W], dy [N, Cout, H, W]"""
    Cout, Cin = w.shape
    w, b, gamma = (t.to(dtype).clone().requires_grad_(True) for t in (w, b, gamma))
    (F.conv2d(g.to(dtype), w.view(Cout, Cin, 1, 1), b) * gamma.view(1, Cout, 1, 1)).backward(dy.to(dtype))
    return dict(dw=w.grad, db=b.grad, dgamma=gamma.grad)


def _dyadic(shape, g, regime):
    """random: multiples of 1/4 in [-2, 2] (rounded normal); integer: integers in [-2, 2].  Products and the sums over the 2 x 2 map and
    N <= 3 images are exact in float32 either way."""
    if regime == 'integer':
        return int_values(shape, g, 2)
    return (torch.randn(shape, generator=g) * 4).round().clamp(-8, 8) / 4


def gram_inputs(g, dy):
    """what the kernels take in place of the maps, computed in float64 and exact in float32 (the host tier checks that):
    G3 [N, Cout, Cin] = sum_p dy g, S3 [Cout] = sum_{n, p} dy, pooled [N, Cin] = mean_p g"""
    G3 = torch.einsum('nohw,nihw->noi', dy.double(), g.double())
    return G3, dy.double().sum((0, 2, 3)), g.double().mean((2, 3))


def sca_inputs(C, N, regime):
    """integer regime: beta and w3 are integers in [-2, 2] too, so ds = sum_co beta W3 G3 and dbsca = sum_n ds are exact"""
    gn = _gen(case_seed('sca', C, N, regime))
    g, dy = _dyadic((N, C, SCA_HW, SCA_HW), gn, regime), _dyadic((N, C, SCA_HW, SCA_HW), gn, regime)
    if regime == 'integer':
        w3, beta = int_values((C, C), gn, 2), int_values((C,), gn, 2)
    else:
        w3, beta = torch.randn(C, C, generator=gn) * 0.2, torch.randn(C, generator=gn)
    b3, bsca = torch.randn(C, generator=gn), torch.randn(C, generator=gn)
    wsca = torch.randn(C, C, generator=gn) * 0.2
    G3, S3, pooled = gram_inputs(g, dy)
    return dict(C=C, N=N, g=g, dy=dy, w3=w3, b3=b3, beta=beta, wsca=wsca, bsca=bsca, G3=G3, S3=S3, pooled=pooled)


def sca_reference(inp):
    args = [inp[k] for k in ('g', 'dy', 'w3', 'b3', 'beta', 'wsca', 'bsca')]
    r, r32 = sca_ref(*args, torch.float64), sca_ref(*args, torch.float32)
    r['e32'] = {k: maxabs(r32[k], r[k]) for k in SCA_OUT}
    r['bar'] = {k: bar(r['e32'][k], r[k]) for k in SCA_OUT}
    return r


def param_inputs(Cout, Cin, extra):
    gn = _gen(case_seed('param', Cout, Cin, extra))
    N = 3
    g, dy = _dyadic((N, Cin, SCA_HW, SCA_HW), gn, 'random'), _dyadic((N, Cout, SCA_HW, SCA_HW), gn, 'random')
    w = torch.randn(Cout + extra, Cin, generator=gn) * 0.2
    b, gamma = torch.randn(Cout + extra, generator=gn), torch.randn(Cout + extra, generator=gn)
    G3, S3, _ = gram_inputs(g, dy)
    return dict(Cout=Cout, Cin=Cin, g=g, dy=dy, w=w, b=b, gamma=gamma, G=G3.sum(0), S=S3)


def param_reference(inp):
    Cout = inp['Cout']
    args = (inp['g'], inp['dy'], inp['w'][:Cout], inp['b'][:Cout], inp['gamma'][:Cout])
    r, r32 = param_ref(*args, torch.float64), param_ref(*args, torch.float32)
    r['e32'] = {k: maxabs(r32[k], r[k]) for k in ('dw', 'db', 'dgamma')}
    r['bar'] = {k: bar(r['e32'][k], r[k]) for k in ('dw', 'db', 'dgamma')}
    return r


# ------------------------------------------------------------------------------------------------------------------ plain sums
PAIR_SUM_ONE_STAGE = [(1, 8), (15, 48), (16, 64), (33, 70), (1024, 32)]                         # (nparts, C)
PAIR_SUM_TWO_STAGE = [(1025, 32), (1300, 48), (2049, 64), (1025, 70), (1030, 128), (1100, 160), (1025, 300)]
PAIR_SUM_CASES = PAIR_SUM_ONE_STAGE + PAIR_SUM_TWO_STAGE
CHANSUM_CASES = [(1, 90, 0), (1, 8191, 0), (3, 2731, 1), (4, 10000, 0)]                          # (N, HW, x is a channel slice); N HW = 90, 8191, 8193, 40000
CHANSUM_C = 5
REGIMES = ('integer', 'random')


def pair_sum_ref(part, dtype, drop_row=None):
    """part [nparts, 2, C] -> (o0 [C], o1 [C], sum |t| [2, C]); drop_row: the planted defect, one partial row left out"""
    p = part.to(dtype)
    if drop_row is not None:
        p = torch.cat([p[:drop_row], p[drop_row + 1:]])
    s = p.sum(0)
    return s[0], s[1], p.abs().sum(0)


def pair_sum_inputs(nparts, C, regime):
    g = _gen(case_seed('pair', nparts, C, regime))
    return int_values((nparts, 2, C), g) if regime == 'integer' else torch.randn(nparts, 2, C, generator=g)


def pair_sum_reference(part, nparts, C):
    o0, o1, at = pair_sum_ref(part, torch.float64)
    a0, a1, _ = pair_sum_ref(part, torch.float32)
    ref = torch.stack([o0, o1])
    e32 = maxabs(torch.stack([a0, a1]), ref)
    return ref, e32, reduced_bar(e32, ref, pair_sum_depth(nparts, C), at)


def channel_sum_ref(x, dtype):
    x = x.to(dtype)
    return x.sum((0, 2, 3)), x.abs().sum((0, 2, 3))


def channel_sum_inputs(N, HW, regime):
    g = _gen(case_seed('chansum', N, HW, regime))
    shape = (N, CHANSUM_C, 1, HW)
    return int_values(shape, g) if regime == 'integer' else torch.randn(shape, generator=g)


def channel_sum_reference(x):
    N, _, _, HW = x.shape
    ref, at = channel_sum_ref(x, torch.float64)
    e32 = maxabs(channel_sum_ref(x, torch.float32)[0], ref)
    return ref, e32, reduced_bar(e32, ref, chansum_depth(N, HW), at)


# (name, N, length, src row stride, dst row stride, src offset in floats): the float4 path needs length, both strides and both pointers
# to be multiples of 4 floats; one length per path runs past the 2048 x 256 threads of the grid
GRID = 2048 * 256
ROWS_CASES = [
    ('float4', 2, 64, 80, 96, 0),
    ('odd_length', 2, 63, 80, 96, 0),
    ('odd_stride', 2, 64, 81, 96, 0),
    ('offset_pointer', 2, 64, 80, 96, 1),
    ('scalar_grid_stride', 1, GRID + 5, GRID + 5, GRID + 8, 0),
    ('float4_grid_stride', 1, 4 * GRID + 8, 4 * GRID + 8, 4 * GRID + 16, 0),
]
ROWS_SENTINEL = 100.0


def rows_path(N, length, src_ns, dst_ns, off):
    return 'rows_kernel' if length % 4 == 0 and src_ns % 4 == 0 and dst_ns % 4 == 0 and off % 4 == 0 else 'rows_scalar_kernel'


def rows_inputs(name, N, length, src_ns, dst_ns, off):
    """integer-valued flat buffers: src [off + N src_ns], dst [N dst_ns] (the rows random, the gaps between them ROWS_SENTINEL)"""
    g = _gen(case_seed('rows', name))
    src = int_values((off + N * src_ns,), g)
    dst = torch.full((N * dst_ns,), ROWS_SENTINEL)
    dst.view(N, dst_ns)[:, :length] = int_values((N, length), g)
    return src, dst


def rows_ref(src, dst, N, length, src_ns, dst_ns, off, add):
    """the float64 result of copy_rows (add = False) / add_rows on the whole dst buffer, gaps included"""
    out = dst.double().clone()
    rows = src.double()[off:off + N * src_ns].view(N, src_ns)[:, :length]
    if add:
        out.view(N, dst_ns)[:, :length] += rows
    else:
        out.view(N, dst_ns)[:, :length] = rows
    return out


# ------------------------------------------------------------------------------------------------- depthwise-gate forward stencils
DW_CASES = [(1, 2, 9, 1028), (1, 2, 40, 2052)]        # (N, C, H, W): W > 1024, two and three column blocks


def dw_inputs(N, C, H, W):
    g = _gen(case_seed('dw', N, C, H, W))
    return dict(t=torch.randn(N, 2 * C, H, W, generator=g), w=torch.randn(2 * C, 1, 3, 3, generator=g) * 0.3,
                b=torch.randn(2 * C, generator=g) * 0.2)


def dw_ref(t, w, b, gate, dtype):
    """depthwise 3 x 3 (pad 1) over the 2C planes, then the gate in dtype: 'mul' (SimpleGate) -> (g, pooled [N, C], mean |g| [N, C]),
    'gelu' (erf GELU of the first half times the second) -> g, 'none' -> the 2C filtered planes"""
    C2 = t.shape[1]
    u = F.conv2d(t.to(dtype), w.to(dtype), b.to(dtype), padding=1, groups=C2)
    u1, u2 = u[:, :C2 // 2], u[:, C2 // 2:]
    if gate == 'mul':
        g = u1 * u2
        return g, g.mean(dim=(2, 3)), g.abs().mean(dim=(2, 3))
    if gate == 'gelu':
        return F.gelu(u1) * u2
    assert gate == 'none', gate
    return u
