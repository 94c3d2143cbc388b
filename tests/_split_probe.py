"""Single-product probe of the split arithmetic: inputs under which EVERY output element of a contraction is one
product a * b -- all other terms of its dot product are exact zeros -- so accumulation order, split-K, tile shape and the summation
inside a matrix instruction contribute nothing and what is left is the error of the product scheme alone:

    bx3: six products of three bf16 planes per operand  lh hl mm mh hm hh      bar 2^-21 per element, relative to |a * b|
    hx2: three products of two fp16 planes per operand        mh hm hh      bar 2^-20
    f32: one fp32 product                                                      bar 2^-23

The bars come from the schemes, not from the kernels: tests/test_split_probe_host.py emulates each scheme on the CPU (2^20 samples)
and asserts that the full scheme stays under bar / 2 while every scheme with ONE product removed exceeds 8 * bar.

A plain helper module (no fixtures): the input builders return (inputs, expected float64, mask of the non-zero outputs); where the mask
is False the output has no non-zero term at all and must be exactly 0.0.  Everything here runs on the CPU.

Values: magnitudes uniform in [0.25, 4) with a random sign, full fp32 mantissas, for both operands -- inside the fp16 window, so one
input set serves all three modes (randn would not: near-zero operands leave the window of the 2-way split)."""
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
