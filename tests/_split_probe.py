"""Single-product probe of the split arithmetic: inputs under which EVERY output element of a contraction is one
product a * b -- all other terms of its dot product are exact zeros -- so accumulation order, split-K, tile shape and the summation
inside a matrix instruction contribute nothing and what is left is the error of the product scheme alone:

    bx3: six products of three bf16 planes per operand  lh hl mm mh hm hh      bar 2^-21 per element, relative to |a * b|
    hx2: three products of two fp16 planes per operand        mh hm hh      bar 2^-20
    f32: one fp32 product                                                      bar 2^-23

The bars come from the schemes, not from the kernels: tests/test_split_probe_host.py emulates each scheme on the CPU (2^20 samples)
and asserts that the full scheme stays under bar / 2 while every scheme with ONE product removed exceeds 8 * bar.

A plain helper module (no fixtures): the input builders return (inputs, expected float64, mask of the non-zero outputs); where the mask
is False the output has no non-zero term at all and must be exactly 0.0.  Everything here runs on the CPU.  The builders of the fused
NAFBlock chains (further down) return what their stage needs on top of that: where the operand of a stage is itself a product formed by
the kernel, its place in the kernel's stored tensor and the weight row that multiplies it, so that the test forms the expectation from
the stored value.

Values: magnitudes uniform in [0.25, 4) with a random sign, full fp32 mantissas, for both operands -- inside the fp16 window, so one
input set serves all three modes (randn would not: near-zero operands leave the window of the 2-way split)."""
import functools
import math

import torch

BAR = {'bx3': 2.0 ** -21, 'hx2': 2.0 ** -20, 'f32': 2.0 ** -23}
PRODUCTS = {'bx3': ('lh', 'hl', 'mm', 'mh', 'hm', 'hh'), 'hx2': ('mh', 'hm', 'hh'), 'f32': ('xx',)}


# ------------------------------------------------------------------ values and the schemes
def values(*shape, seed):
    """fp32 values with magnitude uniform in [0.25, 4), random sign and a full mantissa (drawn in float64, rounded once)"""
    g = torch.Generator().manual_seed(seed)
    mag = 0.25 + 3.75 * torch.rand(*shape, generator=g, dtype=torch.float64)
    sign = torch.randint(0, 2, tuple(shape), generator=g).double() * 2 - 1
    return (mag * sign).float()


def split3_bf16(x):
    """h = rn_bf16(x), m = rn_bf16(x - h), l = rn_bf16(x - h - m): the subtractions are exact in fp32"""
    h = x.bfloat16().float()
    r = x - h
    m = r.bfloat16().float()
    return {'h': h, 'm': m, 'l': (r - m).bfloat16().float()}


def split2_f16(x):
    """h = rn_f16(x), m = rn_f16(x - h)"""
    h = x.half().float()
    return {'h': h, 'm': (x - h).half().float()}


def emulate(a, b, scheme, drop=None):
    """a * b element by element as the scheme forms it: products of the planes (exact in fp32: 8 + 8 or 11 + 11 significand bits)
    accumulated in fp32 in the documented order, small cross terms first.  drop: name of one product left out ('lh': a's l plane times
    b's h plane) -- the wrong kernels the bars must catch."""
    a, b = a.float(), b.float()
    if scheme == 'f32':
        assert drop is None
        return a * b
    pa, pb = (split3_bf16(a), split3_bf16(b)) if scheme == 'bx3' else (split2_f16(a), split2_f16(b))
    assert drop is None or drop in PRODUCTS[scheme]
    acc = torch.zeros_like(a)
    for name in PRODUCTS[scheme]:
        if name != drop:
            acc = acc + pa[name[0]] * pb[name[1]]
    return acc


def max_rel(out, expected, mask):
    """max over the single-product outputs of |out - a * b| / |a * b| (float64)"""
    out = out.detach().cpu().double()
    assert out.shape == expected.shape, (tuple(out.shape), tuple(expected.shape))
    return ((out - expected).abs()[mask] / expected.abs()[mask]).max().item()


def zeros_exact(out, mask):
    """True when every output without a non-zero term is exactly 0.0"""
    out = out.detach().cpu()
    return bool((out[~mask] == 0.0).all())


# ------------------------------------------------------------------ sparse images: one non-zero channel at chosen pixels
def _pixels(H, W, pattern):
    """(ys, xs) of the non-zero pixels.  'all': every pixel; ('lattice', pitch, a, b): y % pitch == a and x % pitch == b;
    'cell2': one pixel in every 2 x 2 cell, its place in the cell cycling through the four taps"""
    if pattern == 'all':
        ys, xs = torch.meshgrid(torch.arange(H), torch.arange(W), indexing='ij')
    elif pattern == 'cell2':
        by, bx = torch.meshgrid(torch.arange(H // 2), torch.arange(W // 2), indexing='ij')
        t = (3 * by + bx) % 4
        ys, xs = 2 * by + t // 2, 2 * bx + t % 2
    else:
        _, pitch, a, b = pattern
        ys, xs = torch.meshgrid(torch.arange(a, H, pitch), torch.arange(b, W, pitch), indexing='ij')
    return ys.reshape(-1), xs.reshape(-1)


def onehot_image(N, C, H, W, pattern, seed):
    """[N, C, H, W] fp32, zero except at the pattern's pixels, where exactly one channel is non-zero: pixel number q of image n (in
    the pattern's raster order) carries channel (7 q + n) mod C.  With at least C pixels in the pattern every channel -- every octet,
    16-channel group and plane slot of the contraction -- is hit in every image (7 and C coprime, asserted)."""
    assert math.gcd(7, C) == 1
    ys, xs = _pixels(H, W, pattern)
    assert ys.numel() >= C, f'{ys.numel()} non-zero pixels do not reach all {C} channels'
    x = torch.zeros(N, C, H, W)
    v = values(N, ys.numel(), seed=seed)
    q = torch.arange(ys.numel())
    for n in range(N):
        c = (7 * q + n) % C
        assert c.unique().numel() == C
        x[n, c, ys, xs] = v[n]
    return x


def best_lattice(H, W, KH, stride, pad, pitch=3):
    """the lattice offset under which most output windows hold a lattice pixel (the windows that hold none hang over the border)"""
    def hit(L, a):
        OL = (L + 2 * pad - KH) // stride + 1
        return sum(any(0 <= o * stride - pad + k < L and (o * stride - pad + k) % pitch == a for k in range(KH)) for o in range(OL))
    return ('lattice', pitch, max(range(pitch), key=lambda a: hit(H, a)), max(range(pitch), key=lambda b: hit(W, b)))


# ------------------------------------------------------------------ expected values: one gathered product per output
def expect_conv(x, w, stride=1, pad=0):
    """conv2d(x, w, stride, pad) of a sparse one-hot x, formed WITHOUT a sum: every non-zero input value is multiplied (in float64:
    exact) into the outputs whose window holds it; an output reached twice is an error of the layout.
    w [Cout, Cin, KH, KH] or per image [N, Cout, Cin, KH, KH] -> (expected [N, Cout, OH, OW] float64, mask)"""
    N, C, H, W = x.shape
    wi = w if w.dim() == 5 else w.unsqueeze(0).expand(N, *w.shape)
    Cout, KH = wi.shape[1], wi.shape[3]
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KH) // stride + 1
    exp = torch.zeros(N, Cout, OH, OW, dtype=torch.float64)
    cnt = torch.zeros(N, OH, OW, dtype=torch.int64)
    n, c, y, xx = x.nonzero(as_tuple=True)
    v = x[n, c, y, xx].double()
    for ky in range(KH):
        for kx in range(KH):
            ny, nx = y + pad - ky, xx + pad - kx
            ok = (ny % stride == 0) & (nx % stride == 0) & (ny >= 0) & (nx >= 0) & (ny // stride < OH) & (nx // stride < OW)
            nn, oy, ox = n[ok], ny[ok] // stride, nx[ok] // stride
            exp[nn, :, oy, ox] = wi[nn, :, c[ok], ky, kx].double() * v[ok, None]
            cnt.index_put_((nn, oy, ox), torch.ones_like(nn), accumulate=True)
    assert cnt.max().item() <= 1, 'an output window holds two non-zero pixels'
    return exp, (cnt == 1)[:, None].expand(N, Cout, OH, OW).clone()


def expect_dgrad(dout, w, stride, pad, H, W):
    """conv_transpose2d(dout, w, stride, pad) onto an H x W image (the data gradient of conv2d(., w)) of a sparse one-hot dout, one
    product per output as in expect_conv.  w [Cout, Cin, KH, KH] -> (expected [N, Cin, H, W] float64, mask)"""
    N, Cout, OH, OW = dout.shape
    Cin, KH = w.shape[1], w.shape[2]
    exp = torch.zeros(N, Cin, H, W, dtype=torch.float64)
    cnt = torch.zeros(N, H, W, dtype=torch.int64)
    n, o, oy, ox = dout.nonzero(as_tuple=True)
    v = dout[n, o, oy, ox].double()
    for ky in range(KH):
        for kx in range(KH):
            y, xx = oy * stride - pad + ky, ox * stride - pad + kx
            ok = (y >= 0) & (xx >= 0) & (y < H) & (xx < W)
            exp[n[ok], :, y[ok], xx[ok]] = w[o[ok], :, ky, kx].double() * v[ok, None]
            cnt.index_put_((n[ok], y[ok], xx[ok]), torch.ones_like(n[ok]), accumulate=True)
    assert cnt.max().item() <= 1, 'a data-gradient pixel is reached by two non-zero output-gradient pixels'
    return exp, (cnt == 1)[:, None].expand(N, Cin, H, W).clone()


# ------------------------------------------------------------------ the builders
def build_conv(N, Cin, Cout, H, W, KH, stride=1, pad=0, seed=0, per_image=False):
    """forward convolution -> ((x, w), expected, mask).  1x1: every pixel one-hot over the channels; 3x3 (stride 1 or 2): non-zero
    pixels on a lattice of pitch 3, so that every window holds at most one and every tap is some output's; 2x2 stride 2: one pixel per
    2 x 2 cell, cycling through the four taps."""
    pattern = 'all' if KH == 1 else 'cell2' if KH == 2 else best_lattice(H, W, KH, stride, pad)
    x = onehot_image(N, Cin, H, W, pattern, seed)
    w = values(*((N,) if per_image else ()), Cout, Cin, KH, KH, seed=seed + 1)
    exp, mask = expect_conv(x, w, stride, pad)
    return (x, w), exp, mask


def dgrad_phases(KH, stride):
    """3x3 stride 2: a data-gradient pixel of an odd row (column) is reached from TWO output rows, so the non-zero output-gradient pixels
    lie on a lattice of pitch 2 and one launch per lattice offset is needed to reach every pixel with a single product (in each launch
    the pixels whose window misses the lattice are exact zeros); every other geometry needs one launch"""
    return 4 if (KH == 3 and stride == 2) else 1


def build_dgrad(N, Cin, Cout, H, W, KH, stride, pad, seed=0, phase=0):
    """data gradient of conv2d(x [N, Cin, H, W], w, stride, pad): the one-hot layouts on dout -> ((dout, w), expected dx, mask).
    1x1 and 2x2 stride 2: every dout pixel (each data-gradient pixel has one tap); 3x3 stride 1: lattice of pitch 3; 3x3 stride 2: lattice
    of pitch 2 at offset `phase` (dgrad_phases)."""
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KH) // stride + 1
    if KH == 1 or (KH == 2 and stride == 2):
        pattern = 'all'
    elif stride == 1:
        pattern = best_lattice(OH, OW, KH, 1, KH - 1 - pad)
    else:
        pattern = ('lattice', 2, phase // 2, phase % 2)
    dout = onehot_image(N, Cout, OH, OW, pattern, seed)
    w = values(Cout, Cin, KH, KH, seed=seed + 1)
    exp, mask = expect_dgrad(dout, w, stride, pad, H, W)
    return (dout, w), exp, mask


def wgrad_phases(stride):
    """stride 2: a tap reads the pixel of a channel only if the pixel's row (column) has the tap's parity, so one launch per parity pair
    is needed for every (channel, tap) to be a single product once (the others are exact zeros in that launch); stride 1: one launch"""
    return 4 if stride == 2 else 1


def build_wgrad(N, Cin, Cout, H, W, KH, stride=1, pad=0, seed=0, phase=0, gate=False, per_image=False):
    """weight gradient dW[o, c, tap] = sum_p dy[o, p] x[c, p + tap]: every input channel c is non-zero at exactly one pixel p(c) of
    exactly one image (of every image with per_image), the p(c) distinct and -- for KH > 1 -- away from the border; dy is dense.
    -> ((x, dy), expected [groups, Cout, Cin, KH, KH], mask).  gate: x is [N, 2 Cin, H, W] with the partner half 1.0 (the SimpleGate
    operand x[:, :Cin] * x[:, Cin:] is then the first half exactly)."""
    OH, OW = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KH) // stride + 1
    groups = N if per_image else 1
    x = torch.zeros(N, Cin, H, W)
    dy = values(N, Cout, OH, OW, seed=seed + 1)
    v = values(N, Cin, seed=seed)
    exp = torch.zeros(groups, Cout, Cin, KH, KH, dtype=torch.float64)
    mask = torch.zeros(groups, Cout, Cin, KH, KH, dtype=torch.bool)
    c = torch.arange(Cin)
    if KH == 1:
        assert math.gcd(7, H * W) == 1 and H * W >= Cin
        cells = None
    else:
        ncy, ncx = (H - 2) // 2, (W - 2) // 2                       # 2 x 2 cells with tops 1, 3, 5, ...: pixels in [1, H - 2]
        assert ncy * ncx >= Cin, 'fewer interior cells than channels'
    for n in range(N):
        own = torch.ones(Cin, dtype=torch.bool) if per_image else (c % N == n)
        if KH == 1:
            p = (7 * c + 3 + 11 * n) % (H * W)
            ys, xs = p // W, p % W
        else:
            k = (c * ((ncy * ncx) // Cin) + n) % (ncy * ncx)
            ys, xs = 1 + 2 * (k // ncx) + (phase // 2 + n) % 2, 1 + 2 * (k % ncx) + (phase % 2 + c) % 2
        assert torch.stack([ys, xs]).unique(dim=1).shape[1] == Cin
        x[n, c[own], ys[own], xs[own]] = v[n, own]
        gi = n if per_image else 0
        for ky in range(KH):
            for kx in range(KH):
                ny, nx = ys + pad - ky, xs + pad - kx
                ok = own & (ny % stride == 0) & (nx % stride == 0) & (ny >= 0) & (nx >= 0) & (ny // stride < OH) & (nx // stride < OW)
                exp[gi][:, c[ok], ky, kx] = dy[n][:, ny[ok] // stride, nx[ok] // stride].double() * v[n, ok].double()
                mask[gi][:, c[ok], ky, kx] = True
    if gate:
        x = torch.cat([x, torch.ones_like(x)], 1)
    return (x, dy), exp, mask


def build_tok(P, N, Kd, seed=0, phase=0):
    """token-major GEMM out[n, p] = sum_k x[p, k] w[n, k]: row p of x is one-hot at k = (p + phase * P) mod Kd, w is dense.
    tok_phases(P, Kd) launches reach every k.  -> ((x [P, Kd], w [N, Kd]), expected [N, P], mask)"""
    k = (torch.arange(P) + phase * P) % Kd
    x = torch.zeros(P, Kd)
    v = values(P, seed=seed)
    x[torch.arange(P), k] = v
    w = values(N, Kd, seed=seed + 1)
    exp = w[:, k].double() * v.double()[None]
    return (x, w), exp, torch.ones(N, P, dtype=torch.bool)


def tok_phases(P, Kd):
    return -(-Kd // P)


# ------------------------------------------------------------------ the fused NAFBlock chains (csrc/tdr_nafblock_chain.h)
# Every GEMM stage of the chain kernels behind a one-hot operand.  The operands of the inner stages are formed inside the kernel, so they
# are steered from the outside: the LayerNorm bias and the conv4 bias carry a chosen one-hot vector to conv1 / conv4 / conv5 of the forward
# chains (lnw = 0 makes xn = lnb exactly, a zero tile makes t4 = b4 exactly); the saved tensors t4, y, mu, rs and lnw are plain inputs of the
# backward chains.  Between the accumulator and the stored value only exact fp32 operations remain (+ 0, * 1, * 2^-k), so the bars are BAR[cls]
# as they stand.  An expectation that is the same for every image and pixel has shape [1, M, 1, 1] (or [N, M, 1, 1]) and broadcasts.
CHAIN_EPS = 1e-6
WINDOW = (0.25, 4.0)


def in_window(t):
    """True when every non-zero element has its magnitude in the fp16 window [0.25, 4) of `values`"""
    m = t.abs()[t != 0]
    return bool(((m >= WINDOW[0]) & (m < WINDOW[1])).all())


def pow2_toward_one(x):
    """2^e with |x| 2^e in [2^-0.5, 2^0.5]: the factor that brings a product of two window values (1/16 ... 16) back into the window"""
    return torch.pow(2.0, -torch.round(torch.log2(x.double().abs())))


def values_with_product_in_window(w, seed):
    """u with a full mantissa, |u| in the window and |w u| in the window as well, element by element (w in the window): magnitude uniform
    in [max(1/4, 1/(4|w|)), min(4, 4/|w|)) shrunk by 1 % at both ends, random sign"""
    g = torch.Generator().manual_seed(seed)
    aw = w.double().abs()
    lo, hi = torch.clamp(0.25 / aw, min=0.25) * 1.01, torch.clamp(4.0 / aw, max=4.0) * 0.99
    mag = lo + (hi - lo) * torch.rand(w.shape, generator=g, dtype=torch.float64)
    sign = torch.randint(0, 2, tuple(w.shape), generator=g).double() * 2 - 1
    return (mag * sign).float()


@functools.lru_cache(maxsize=None)
def chain_image(N, C, H, W, seed):
    """dense `values` [N, C, H, W], built once per shape and only read"""
    return values(N, C, H, W, seed=seed)


@functools.lru_cache(maxsize=None)
def chain_weights(C, seed=40):
    """conv1 / conv4 [2C, C, 1, 1], conv3 / conv5 / the TLSC channel attention [C, C, 1, 1]: dense `values`, built once and only read"""
    return {'w1': values(2 * C, C, 1, 1, seed=seed), 'w3': values(C, C, 1, 1, seed=seed + 1), 'w4': values(2 * C, C, 1, 1, seed=seed + 2),
            'w5': values(C, C, 1, 1, seed=seed + 3), 'wsca': values(C, C, 1, 1, seed=seed + 4)}


def _mat(w):
    return w.view(w.shape[0], w.shape[1]).double()


def bias_route(C, k, seed=50):
    """LayerNorm parameters that put v e_k in front of the GEMM behind the norm: lnw = 0, lnb = v[k] e_k -> (lnw, lnb, v[k])"""
    v = values(C, seed=seed)
    lnb = torch.zeros(C)
    lnb[k] = v[k]
    return torch.zeros(C), lnb, v[k]


def mod_rows(N, C2, shift_only_upper=False):
    """power-of-two modulation rows [N, C2] of the text-modulated chains: a = +-2^e, e = -1, 1, 2 with c mod 3, the sign alternating over channels and
    images, b = +-2^(c mod 2) (shift_only_upper: b is a r on the upper half, r = 2^(c mod 2), and zero on the lower one -- a lower-half
    shift would make every gate channel non-zero)"""
    c = torch.arange(C2)
    n = torch.arange(N)[:, None]
    a = torch.pow(2.0, torch.tensor([-1.0, 1.0, 2.0])[c % 3])[None] * (1.0 - 2.0 * ((n + c[None]) % 2))
    if not shift_only_upper:
        return a, torch.pow(2.0, (c % 2).float())[None] * (1.0 - 2.0 * ((n + c[None] // 2) % 2))
    b = a * torch.pow(2.0, (c % 2).float())[None]
    b[:, :C2 // 2] = 0.0
    return a, b


def build_head_conv1(N, C, H, W, k, seed=0):
    """naf_head_fwd, conv1 at K index k: xn = (x - mu) rstd 0 + lnb = v e_k at every pixel for any finite x, b1 = 0 ->
    t1[o, p] = W1[o, k] v.  -> (inputs, expected [1, 2C, 1, 1], mask)"""
    w1 = chain_weights(C)['w1']
    lnw, lnb, v = bias_route(C, k)
    inputs = {'x': chain_image(N, C, H, W, seed + 60), 'lnw': lnw, 'lnb': lnb, 'b1': torch.zeros(2 * C), 'w1': w1}
    exp = (_mat(w1)[:, k] * v.double()).view(1, 2 * C, 1, 1)
    return inputs, exp, torch.ones(1, 2 * C, 1, 1, dtype=torch.bool)


def build_tail_conv4(N, C, H, W, k, seed=0):
    """naf_tail_fwd, conv4 at K index k: g = 0 and b3 = 0 make y = x, the bias route on norm2 makes yn = v e_k, b4 = 0 ->
    t4[o, p] = W4[o, k] v for all 2C rows.  -> (inputs, expected [1, 2C, 1, 1], mask)"""
    wts = chain_weights(C)
    lnw, lnb, v = bias_route(C, k)
    z, one = torch.zeros(C), torch.ones(C)
    inputs = {'g': torch.zeros(N, C, H, W), 'sca': torch.ones(N, C), 'x': chain_image(N, C, H, W, seed + 61), 'b3': z, 'beta': one, 'lnw': lnw,
              'lnb': lnb, 'b4': torch.zeros(2 * C), 'b5': z, 'gamma': one, 'w3': wts['w3'], 'w4': wts['w4'], 'w5': wts['w5']}
    exp = (_mat(wts['w4'])[:, k] * v.double()).view(1, 2 * C, 1, 1)
    return inputs, exp, torch.ones(1, 2 * C, 1, 1, dtype=torch.bool)


def build_tail_conv5(N, C, H, W, j, c_out=None, mod=False, seed=0):
    """naf_tail_fwd, conv5 at K index j: x = 0, g = 0, b3 = 0, lnw = lnb = 0 make y = yn = 0 and t4 = b4 exactly (with the modulation rows
    of dyn_tail_infer: t4 = b4 a2 + b2, powers of two times b4 and a sum of two equal powers of two -- exact, fused or not).  b4 is
    non-zero at j and C + j, so the gate operand is one-hot at j with the value fl32(t4[j] t4[C + j]); one factor is a power of two, chosen so
    that the product stays in the window.  b5 = 0, gamma = 1, y = 0: out[o, p] = W5[o, j] operand, rows below c_out.
    -> (inputs with 't4' (the exact expected t4 rows [N, 2C]) and 'operand' [N], expected [N, c_out, 1, 1], mask)"""
    c_out = C if c_out is None else c_out
    wts = chain_weights(C)
    a2, b2 = mod_rows(N, 2 * C, shift_only_upper=True) if mod else (torch.ones(N, 2 * C), torch.zeros(N, 2 * C))
    v = values(C, seed=seed + 70)[j].double()
    r = 2.0 ** (j % 2)
    up = r * a2[:, C + j].double() + b2[:, C + j].double()                    # t4[C + j] per image: +-2^e, the same magnitude in every image
    lo_scale = a2[:, j].double().abs() * up.abs()
    assert (lo_scale == lo_scale[0]).all() and torch.log2(lo_scale[0]) % 1 == 0
    adj = 1.0 if j % 2 == 0 else (2.0 if abs(v) < 2 else 0.5)                 # a non-trivial power of two that keeps |v| adj in the window
    b4 = torch.zeros(2 * C)
    b4[j], b4[C + j] = float(v * adj / lo_scale[0]), r
    t4 = b4.double()[None] * a2.double() + b2.double()
    assert torch.equal(t4.float().double(), t4)
    gate = t4[:, :C].float() * t4[:, C:].float()                               # the IEEE product the kernel forms
    assert torch.equal(gate.double(), t4[:, :C] * t4[:, C:]) and ((gate != 0).sum(1) == 1).all() and in_window(gate)
    z, one = torch.zeros(C), torch.ones(C)
    zimg = torch.zeros(N, C, H, W)
    inputs = {'g': zimg, 'sca': torch.ones(N, C), 'x': zimg, 'b3': z, 'beta': one, 'lnw': z, 'lnb': z, 'b4': b4, 'b5': z, 'gamma': one,
              'w3': wts['w3'], 'w4': wts['w4'], 'w5': wts['w5'], 'a2': a2, 'b2': b2, 't4': t4.float(), 'operand': gate[:, j]}
    exp = _mat(wts['w5'])[None, :c_out, j] * gate[:, j].double()[:, None]
    return inputs, exp.view(N, c_out, 1, 1), torch.ones(N, c_out, 1, 1, dtype=torch.bool)


def build_tail_bwd_conv53(N, C, H, W, c_out=None, seed=0):
    """naf_tail_bwd, conv5^T and conv3^T in one launch: dout one-hot over its c_out channels at every pixel, gamma = 1, t4 = 1 (both halves
    of dt4 are W5^T dout), lnw = 0 with y = mu = 0 and rs = 1 (dy = (0 - 0 - 0) 1 + dout = dout on the first c_out rows, zero above),
    beta = 1, sca = 1 (dgp = W3^T dy).  -> (inputs, {'dt4', 'dy', 'dgp': (expected, mask)})"""
    c_out = C if c_out is None else c_out
    wts = chain_weights(C)
    dout = onehot_image(N, c_out, H, W, 'all', seed + 80)
    inputs = {'dout': dout, 'gamma': torch.ones(C), 't4': torch.ones(N, 2 * C, H, W), 'y': torch.zeros(N, C, H, W), 'mu': torch.zeros(N, H * W),
              'rs': torch.ones(N, H * W), 'lnw': torch.zeros(C), 'beta': torch.ones(C), 'sca': torch.ones(N, C),
              'w5': wts['w5'][:c_out].contiguous(), 'w4': wts['w4'], 'w3': wts['w3']}
    e5, m5 = expect_dgrad(dout, inputs['w5'], 1, 0, H, W)
    e3, m3 = expect_dgrad(dout, wts['w3'][:c_out], 1, 0, H, W)
    dy = torch.cat([dout, torch.zeros(N, C - c_out, H, W)], 1)
    return inputs, {'dt4': (torch.cat([e5, e5], 1), torch.cat([m5, m5], 1)), 'dy': (dy.double(), dy != 0), 'dgp': (e3, m3)}


PARTIAL_LAUNCHES = 16


def partial_layout(N, C, H, W, launch):
    """one (image, K index, pixel) per 64-pixel workgroup b of the launch: K index (16 (b + launch) + launch) mod 2C -- the sixteen
    launches reach all 2C -- at pixel slot (4 launch + b) mod 64 of the workgroup -- all 64 slots occur.  -> (n, j, p) index vectors"""
    assert H * W % 64 == 0 and (N * (H * W // 64)) * 16 == 2 * C
    b = torch.arange(N * (H * W // 64))
    j = (16 * (b + launch) + launch) % (2 * C)
    return b // (H * W // 64), j, (b % (H * W // 64)) * 64 + (4 * launch + b) % 64


def _ln_inputs(N, C, H, W, yhat, seed):
    """(y, mu, rs) with (y - mu) rs = yhat exactly in fp32: mu is integer valued, y = mu + yhat, rs = 1"""
    mu = torch.randint(-3, 4, (N, H * W), generator=torch.Generator().manual_seed(seed)).float()
    return (mu.view(N, 1, H, W) + float(yhat)).expand(N, C, H, W).contiguous(), mu, torch.ones(N, H * W)


def build_head_bwd_partials(N, C, H, W, launch, yhat=0, seed=0):
    """naf_head_bwd, conv1^T (K = 2C) through the per-workgroup LayerNorm-gradient partials: dt1 is non-zero at one (channel j, pixel p*)
    per workgroup (partial_layout), so its gb row sum_pixels dxn[c, p] is W1[j, c] dt1[j, p*] -- the other 63 terms are exact zeros -- and
    its gw row is the same times yhat (0 or 1).  lnw = 0: dx = res.  -> (inputs, expected gb [workgroups, C], mask)"""
    w1 = chain_weights(C)['w1']
    n, j, p = partial_layout(N, C, H, W, launch)
    val = values(n.numel(), seed=seed + 90 + launch)
    dt1 = torch.zeros(N, 2 * C, H * W)
    dt1[n, j, p] = val
    y, mu, rs = _ln_inputs(N, C, H, W, yhat, seed + 91)
    inputs = {'dt1': dt1.view(N, 2 * C, H, W), 'x': y, 'mu': mu, 'rs': rs, 'lnw': torch.zeros(C), 'res': chain_image(N, C, H, W, seed + 92), 'w1': w1}
    exp = _mat(w1)[j] * val.double()[:, None]
    return inputs, exp, torch.ones_like(exp, dtype=torch.bool)


def build_tail_bwd_partials(N, C, H, W, launch, yhat=0, seed=0):
    """naf_tail_bwd, conv4^T (K = 2C) through the partials: dout one-hot at every pixel, t4 non-zero at one (j, p*) per workgroup only, so
    dt4 is non-zero only at ((j + C) mod 2C, p*), where it is (W5[o(p*), j mod C] dout[o(p*), p*]) t4[j, p*]; t4 there is the power of two that
    brings that product into the window.  The gb row of the workgroup is W4[(j + C) mod 2C, c] times the kernel's own stored dt4 value.
    -> (inputs, (n, j', p) of the operand, expected dt4 [N, 2C, H, W] with its mask, weight rows W4[j'] [workgroups, C] float64)"""
    wts = chain_weights(C)
    n, j, p = partial_layout(N, C, H, W, launch)
    dout = onehot_image(N, C, H, W, 'all', seed + 100 + launch)
    d = dout.view(N, C, H * W)
    o = (d[n, :, p] != 0).float().argmax(1)
    dg2 = _mat(wts['w5'])[o, j % C] * d[n, o, p].double()
    t4 = torch.zeros(N, 2 * C, H * W)
    sign = 1.0 - 2.0 * ((j + launch) % 2).double()
    t4[n, j, p] = (pow2_toward_one(dg2) * sign).float()
    jp = (j + C) % (2 * C)
    edt4 = torch.zeros(N, 2 * C, H * W, dtype=torch.float64)
    edt4[n, jp, p] = dg2 * t4[n, j, p].double()
    y, mu, rs = _ln_inputs(N, C, H, W, yhat, seed + 101)
    inputs = {'dout': dout, 'gamma': torch.ones(C), 't4': t4.view(N, 2 * C, H, W), 'y': y, 'mu': mu, 'rs': rs, 'lnw': torch.zeros(C),
              'w5': wts['w5'], 'w4': wts['w4']}
    edt4 = edt4.view(N, 2 * C, H, W)
    return inputs, (n, jp, p), (edt4, edt4 != 0), _mat(wts['w4'])[jp]


def dy_route_rows(C):
    """the LayerNorm weight's hot row of each launch of the dy route: one per wave (32 rows), at a different place in each"""
    return [32 * w + (11 * w + 5) % 32 for w in range(C // 32)]


def build_head_bwd_dy(N, C, H, W, k, seed=0):
    """naf_head_bwd, conv1^T at EVERY pixel through dx: dt1 one-hot over its 2C channels at every pixel, lnw = e_k, x = mu (yhat = 0), rs = 1,
    res = 0.  Then g = dxn lnw is dxn[k] at row k and zero elsewhere, mean_c(g yhat) = 0, mean_c(g) = dxn[k, p] / C (one non-zero term, a
    power-of-two scaling), and for every row c != k: dx[c, p] = (0 - 0 - dxn[k, p] / C) 1 + 0 = -W1[j(p), k] dt1[j(p), p] / C.
    -> (inputs, expected [N, 1, H, W], mask [N, C, H, W]: every row but k)"""
    w1 = chain_weights(C)['w1']
    dt1 = onehot_image(N, 2 * C, H, W, 'all', seed + 110 + k)
    y, mu, rs = _ln_inputs(N, C, H, W, 0, seed + 111)
    lnw = torch.zeros(C)
    lnw[k] = 1.0
    inputs = {'dt1': dt1, 'x': y, 'mu': mu, 'rs': rs, 'lnw': lnw, 'res': torch.zeros(N, C, H, W), 'w1': w1}
    dxn, m = expect_dgrad(dt1, w1, 1, 0, H, W)
    assert m.all()
    mask = torch.ones(N, C, H, W, dtype=torch.bool)
    mask[:, k] = False
    return inputs, -dxn[:, k:k + 1] / C, mask


def build_tail_bwd_dy(N, C, H, W, k, seed=0):
    """naf_tail_bwd, conv4^T at EVERY pixel through dy: dout one-hot (channel o(p)) and t4 non-zero at one channel j(p) of its 2C per pixel --
    a power of two, as in build_tail_bwd_partials -- so dt4 is one-hot at j'(p) = (j(p) + C) mod 2C; lnw = e_k, y = mu, rs = 1.  The skip
    gradient of the tail is dout itself, so dy[c, p] = -W4[j'(p), k] dt4[j'(p), p] / C on every row c outside {k, o(p)} (row o(p) adds dout with
    a rounding and is left out; the pixels all stay).
    -> (inputs, (n, j', p) of the operands, expected dt4 with its mask, W4[j'(p), k] [N, 1, H, W] float64, mask of the rows)"""
    wts = chain_weights(C)
    HW = H * W
    dout = onehot_image(N, C, H, W, 'all', seed + 120 + k)
    d = dout.view(N, C, HW)
    n = torch.arange(N).repeat_interleave(HW)
    p = torch.arange(HW).repeat(N)
    o = (d != 0).float().argmax(1).reshape(-1)
    j = (7 * p + n + 3 * k) % (2 * C)
    dg2 = _mat(wts['w5'])[o, j % C] * d[n, o, p].double()
    t4 = torch.zeros(N, 2 * C, HW)
    t4[n, j, p] = (pow2_toward_one(dg2) * (1.0 - 2.0 * ((p + n) % 2).double())).float()
    jp = (j + C) % (2 * C)
    edt4 = torch.zeros(N, 2 * C, HW, dtype=torch.float64)
    edt4[n, jp, p] = dg2 * t4[n, j, p].double()
    y, mu, rs = _ln_inputs(N, C, H, W, 0, seed + 121)
    lnw = torch.zeros(C)
    lnw[k] = 1.0
    inputs = {'dout': dout, 'gamma': torch.ones(C), 't4': t4.view(N, 2 * C, H, W), 'y': y, 'mu': mu, 'rs': rs, 'lnw': lnw, 'w5': wts['w5'],
              'w4': wts['w4']}
    mask = dout == 0
    mask[:, k] = False
    edt4 = edt4.view(N, 2 * C, H, W)
    return inputs, (n, jp, p), (edt4, edt4 != 0), _mat(wts['w4'])[jp, k].view(N, 1, H, W), mask


def build_local_stages(N, C, H, W, seed=0):
    """naf_tail_infer_local with gamma = 0 (out = y): the conv3 stage alone -- pooled = 0 and bsca = 1 make the attention map 1.0, g is
    one-hot, y = W3 g -- and the wsca stage in front of it -- pooled one-hot (channel c(p), value u), bsca = 0, g = 1.0 at ONE channel h(p), so
    that conv3's operand is the single product s = Wsca[h(p), c(p)] u there and y[o, p] = W3[o, h(p)] s: two single products in a chain, u drawn
    with a full mantissa so that u and Wsca[h, c] u both stay in the window.  -> {'conv3' | 'wsca': (inputs, expected y, mask)}"""
    wts = chain_weights(C)
    zimg, z, one = torch.zeros(N, C, H, W), torch.zeros(C), torch.ones(C)
    # (lnw = lnb = 0 and b4 = 0: conv4 and conv5 run on zero operands, so that out = (0 + 0) 0 + y whatever the range of y)
    common = {'x': zimg, 'b3': z, 'beta': one, 'lnw': z, 'lnb': z, 'b4': torch.zeros(2 * C), 'b5': z, 'gamma': z, 'w3': wts['w3'], 'w4': wts['w4'],
              'w5': wts['w5'], 'wsca': wts['wsca']}
    g = onehot_image(N, C, H, W, 'all', seed + 130)
    e3, m3 = expect_conv(g, wts['w3'])
    conv3 = (dict(common, g=g, pooled=zimg, bsca=one), e3, m3)
    HW = H * W
    n = torch.arange(N).repeat_interleave(HW)
    p = torch.arange(HW).repeat(N)
    c, h = (7 * p + n) % C, (11 * p + 5 * n + 3) % C
    ws = _mat(wts['wsca'])[h, c]
    u = values_with_product_in_window(ws, seed + 131)
    pooled, gh = torch.zeros(N, C, HW), torch.zeros(N, C, HW)
    pooled[n, c, p] = u
    gh[n, h, p] = 1.0
    s = (ws * u.double()).view(N, HW)
    assert in_window(u) and in_window(s)
    exp = (_mat(wts['w3'])[:, h].t().reshape(N, HW, C).permute(0, 2, 1) * s[:, None]).reshape(N, C, H, W)
    wsca = (dict(common, g=gh.view(N, C, H, W), pooled=pooled.view(N, C, H, W), bsca=z), exp, torch.ones(N, C, H, W, dtype=torch.bool))
    return {'conv3': conv3, 'wsca': wsca}


def coverage(masks):
    """share of the outputs that are a single product in at least one of the launches of a case"""
    u = masks[0].clone()
    for m in masks[1:]:
        u |= m
    return u.double().mean().item()


# ------------------------------------------------------------------ the shapes of tests/test_hip_split_probe.py
# (kept here so that tests/test_split_probe_host.py can check every one of them without a GPU)
CONV1X1_CFG_SHAPE = (2, 520, 200, 20, 36, 1, 1, 0)             # the shape of test_conv1x1_every_tile_configuration
CONV3X3_CFG_SHAPE = (2, 72, 136, 24, 40, 3, 1, 1)              # ... of test_conv3x3_every_tile_configuration
CONV_FWD_SHAPES = [  # N, Cin, Cout, H, W, KH, stride, pad
    (1, 40, 72, 16, 36, 1, 1, 0), (1, 204, 72, 16, 36, 1, 1, 0), (2, 256, 96, 24, 40, 1, 1, 0),
    (1, 3, 8, 32, 48, 3, 1, 1), (1, 20, 12, 13, 21, 3, 1, 1), (2, 16, 32, 32, 32, 3, 2, 1), (2, 16, 32, 32, 32, 2, 2, 0)]
CONV_PER_IMAGE_SHAPE = (3, 72, 40, 16, 20, 1, 1, 0)
GATE_SHAPE = (2, 32, 32, 16, 32, 1, 1, 0)
DGRAD_SHAPES = [     # the shapes of test_conv_data_gradient (N = 2)
    (2, 32, 64, 16, 16, 1, 1, 0), (2, 16, 24, 20, 28, 3, 1, 1), (2, 64, 64, 32, 32, 3, 1, 1), (2, 16, 32, 32, 32, 2, 2, 0),
    (2, 16, 32, 32, 48, 3, 2, 1), (2, 8, 16, 16, 16, 3, 2, 1)]
P16_CONV_SHAPES = [(2, 48, 32, 19, 45, 3, 1, 1), (2, 32, 64, 32, 32, 3, 1, 1)]
WGRAD_SHAPES = [     # N, Cin, Cout, H, W, KH, stride, pad, gate, per_image
    (2, 32, 64, 64, 64, 1, 1, 0, False, False), (1, 96, 72, 40, 40, 1, 1, 0, False, False), (2, 256, 512, 32, 32, 1, 1, 0, False, False),
    (3, 32, 32, 16, 16, 1, 1, 0, True, False), (3, 32, 32, 16, 16, 1, 1, 0, False, True), (3, 96, 80, 32, 40, 1, 1, 0, True, True),
    (2, 32, 32, 32, 32, 3, 1, 1, False, False), (1, 8, 8, 13, 17, 3, 1, 1, False, False),
    (2, 32, 64, 64, 64, 3, 2, 1, False, False), (1, 72, 80, 40, 80, 3, 2, 1, False, False),
    (2, 32, 64, 64, 64, 2, 2, 0, False, False)]
WGRAD_GROUP_SHAPE = (2, 128, 256, 32, 32, 1, 1, 0, False, False)
WGRAD_P16_SHAPES = [(1, 32, 32, 16, 32, 3, 1, 1, False, False), (1, 16, 48, 19, 45, 3, 1, 1, False, False)]
TOK3_SHAPES = [(280, 384, 768), (280, 768, 160), (4104, 384, 768), (4104, 768, 160)]      # P, N, K of test_tok16x3_kernels_against_torch
TOK2_SHAPES = [(152, 384, 1280), (152, 1280, 160)]                                        # ... of test_tok16x2_kernels_against_torch
CHAIN_SHAPES = [(2, 32, 8, 16), (2, 64, 16, 16), (2, 128, 16, 32), (2, 256, 32, 32)]      # N, C, H, W: HW = 64 * (C / 16)
