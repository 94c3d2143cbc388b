"""Single-product probe of every matrix-core contraction that a one-hot operand can reach (tests/_split_probe.py), through
the kernels.py / engine.py wrappers.  Each output element is ONE product a * b (the other terms of its dot product are exact zeros), so
the only error left is that of the product scheme: six products of bf16 triples (bx3, bar 2^-21 per element), three of fp16 pairs (hx2,
2^-20), one fp32 product (f32, 2^-23).  A kernel that runs five of the six products, wires a plane pair to the wrong slot of one tile
configuration or skips the l plane of a tail group exceeds its bar 16x or more (tests/test_split_probe_host.py); the parity tests of the
same kernels (2e-5 ... 1e-4 against torch fp32) do not see it.  Every case asserts the shape, exact zeros where no term is non-zero, and
max |out - a * b| / |a * b| <= bar against the float64 product, and prints `probe <kernel> <cfg / shape> <math>: max rel ... (bar ...)`.

The bar of a launch is that of the arithmetic it is documented to run: under hx2 the data gradients and the grouped 1x1 weight
gradients outside a loss-scaled pass (kernels.GRAD_SCALED off) stay on the bf16 triples and are pinned at the bx3 bar, inside one at the
hx2 bar; conv_wgrad 1x1 with kernels.WGRAD_1X1_BX3 off is the exact kernel in every mode and is pinned at the f32 bar.

The fused NAFBlock chains: their conv3 stage is probed here through the saved tensor y (test_chain_conv3_stage); every other GEMM stage
-- conv1, conv4, conv5, the data gradients conv5^T, conv4^T, conv3^T, conv1^T of the backward chains, the forward-only and text-modulated
twins and the channel-attention GEMM of the TLSC tail -- is probed in tests/test_hip_chain_probe.py.  Their operands are formed inside the
kernel, so they are steered from the outside: the LayerNorm bias (lnw = 0, lnb = v e_k) and the conv4 bias place a one-hot vector in front of
the forward stages, and the saved tensors t4, y, mu, rs are plain inputs of the backward chains.
Left out, and why: tok16_gemm (a single fp16 product by design); the dilated search convolutions (packed math='f32': exact by construction).
wgrad1x1_group takes problems of ONE shape per launch, so its three problems differ in their data, not in C."""
import contextlib
import functools

import pytest
import torch

import _split_probe as SP

pytestmark = pytest.mark.gpu

MODES = ['bx3', 'hx2', 'f32']
# (mode, loss-scaled pass, arithmetic class the data-gradient packs are documented to have)
DGRAD_MODES = [('bx3', False, 'bx3'), ('hx2', False, 'bx3'), ('hx2', True, 'hx2'), ('f32', False, 'f32')]


@contextlib.contextmanager
def arithmetic(mode, grad_scaled=False, wgrad_1x1_bx3=True):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels as K
    prev, prev1 = K.MATH, K.WGRAD_1X1_BX3
    K.set_math(mode)
    K.WGRAD_1X1_BX3 = wgrad_1x1_bx3
    prev_scaled = K.set_grad_scaled(grad_scaled)
    try:
        yield K
    finally:
        K.set_math(prev)
        K.WGRAD_1X1_BX3 = prev1
        K.set_grad_scaled(prev_scaled)


def dev(t):
    return t.cuda().contiguous()


def sid(shape):
    return 'x'.join(str(int(v)) for v in shape)


def verdict(kernel, tag, math, cls, runs):
    """runs: [(out, expected, mask)] -- the launches of one case.  Shape, exact zeros, max rel <= bar of the class."""
    worst = 0.0
    for out, exp, mask in runs:
        assert tuple(out.shape) == tuple(exp.shape), (kernel, tag, tuple(out.shape), tuple(exp.shape))
        assert SP.zeros_exact(out, mask), f'{kernel} {tag} {math}: an output without a non-zero term is not exactly 0.0'
        worst = max(worst, SP.max_rel(out, exp, mask))
    bar = SP.BAR[cls]
    print(f'probe {kernel} {tag} {math}: max rel {worst:.2e} (bar {bar:.2e})')
    assert worst <= bar, (kernel, tag, math, worst, bar)


# the inputs and their float64 expectations are built once per shape and only read
@functools.lru_cache(maxsize=None)
def conv_case(shape, per_image=False):
    return SP.build_conv(*shape, seed=3, per_image=per_image)


@functools.lru_cache(maxsize=None)
def dgrad_case(shape, phase=0):
    return SP.build_dgrad(*shape, seed=5, phase=phase)


@functools.lru_cache(maxsize=None)
def wgrad_case(shape, phase=0, seed=7):
    N, Cin, Cout, H, W, KH, st, pd, gate, per_image = shape
    return SP.build_wgrad(N, Cin, Cout, H, W, KH, st, pd, seed=seed, phase=phase, gate=gate, per_image=per_image)


# ------------------------------------------------------------------ conv_forward
def _forward(K, shape, **kw):
    N, Cin, Cout, H, W, KH, st, pd = shape
    (x, w), exp, mask = conv_case(shape)
    wp, mp, *_ = K.pack_weights(dev(w), K.PACK_FWD)
    return K.conv_forward(dev(x), wp, mp, Cout, KH, stride=st, pad=pd, **kw), exp, mask


@pytest.mark.parametrize('cfg', [1, 2, 3, 4, 5])
@pytest.mark.parametrize('mode', MODES)
def test_conv1x1_every_tile_configuration(mode, cfg):
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    with arithmetic(mode) as K:
        lib.tdr_conv_force_cfg(1, cfg)
        try:
            run = _forward(K, SP.CONV1X1_CFG_SHAPE)
        finally:
            lib.tdr_conv_force_cfg(1, 0)
        verdict('conv_forward_1x1', f'cfg{cfg} {sid(SP.CONV1X1_CFG_SHAPE)}', mode, mode, [run])


@pytest.mark.parametrize('cfg', [1, 2, 3, 4])
@pytest.mark.parametrize('mode', MODES)
def test_conv3x3_every_tile_configuration(mode, cfg):
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    with arithmetic(mode) as K:
        lib.tdr_conv_force_cfg(3, cfg)
        try:
            run = _forward(K, SP.CONV3X3_CFG_SHAPE)
        finally:
            lib.tdr_conv_force_cfg(3, 0)
        verdict('conv_forward_3x3', f'cfg{cfg} {sid(SP.CONV3X3_CFG_SHAPE)}', mode, mode, [run])


@pytest.mark.parametrize('shape', SP.CONV_FWD_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', MODES)
def test_conv_forward_unforced(mode, shape):
    """1x1 below and above four K stages with a partial last octet / group, 3x3 with Cin < 8 and ragged channels, stride 2, 2x2 stride 2"""
    with arithmetic(mode) as K:
        verdict(f'conv_forward_{shape[5]}x{shape[5]}s{shape[6]}', sid(shape), mode, mode, [_forward(K, shape)])


@pytest.mark.parametrize('mode', MODES)
def test_conv_forward_per_image_weights(mode):
    """one weight matrix per image (wp_ns: MDTA's attn v, the per-word Linears of the Mapper)"""
    shape = SP.CONV_PER_IMAGE_SHAPE
    N, Cin, Cout, H, W, KH, st, pd = shape
    (x, w), exp, mask = conv_case(shape, True)
    with arithmetic(mode) as K:
        wp, mp, per = K.pack_weights_grouped(dev(w.view(N, Cout, Cin)), K.PACK_FWD)
        out = K.conv_forward(dev(x), wp, mp, Cout, 1, wp_ns=per)
        verdict('conv_forward_1x1_wp_ns', sid(shape), mode, mode, [(out, exp, mask)])


@pytest.mark.parametrize('mode', MODES)
def test_conv_forward_gate_operand(mode):
    """gate=True: the operand is x[:, :C] * x[:, C:], formed while staging; the partner half is 1.0, so the product stays single"""
    shape = SP.GATE_SHAPE
    N, C, Cout, H, W, *_ = shape
    (x, w), exp, mask = conv_case(shape)
    with arithmetic(mode) as K:
        wp, mp, *_ = K.pack_weights(dev(w), K.PACK_FWD)
        out = K.conv_forward(dev(torch.cat([x, torch.ones_like(x)], 1)), wp, mp, Cout, 1, gate=True)
        verdict('conv_forward_1x1_gate', sid(shape), mode, mode, [(out, exp, mask)])


@pytest.mark.parametrize('mode,scaled,cls', DGRAD_MODES)
def test_conv_forward_gatebwd_epilogue(mode, scaled, cls):
    """EPI_GATEBWD: dt4 = [u * t4[:, C:], u * t4[:, :C]] with u = W^T dout; t4 = 1.0 and the input scale 1.0 keep each half at u"""
    shape = SP.GATE_SHAPE
    N, C, Cout, H, W, *_ = shape
    (dout, w), exp, mask = dgrad_case(shape)
    with arithmetic(mode, grad_scaled=scaled) as K:
        wp, mp, *_ = K.pack_weights(dev(w), K.PACK_DGRAD_S1)
        out = K.conv_forward(dev(dout), wp, mp, C, 1, epi=K.EPI_GATEBWD, kscale=torch.ones(Cout, device='cuda'),
                             aux=torch.ones(N, 2 * C, H, W, device='cuda'))
        verdict('conv_forward_1x1_gatebwd', sid(shape) + ('-scaled' if scaled else ''), mode, cls,
                [(out, torch.cat([exp, exp], 1), torch.cat([mask, mask], 1))])


# ------------------------------------------------------------------ data gradients through engine.conv_bwd
@pytest.mark.parametrize('shape', SP.DGRAD_SHAPES, ids=sid)
@pytest.mark.parametrize('mode,scaled,cls', DGRAD_MODES)
def test_conv_data_gradient(mode, scaled, cls, shape):
    """PACK_DGRAD_S1 / PACK_DGRAD_2X2S2 / PACK_DGRAD_3X3S2 (3x3 stride 2: one launch per lattice offset, _split_probe.dgrad_phases)"""
    from textualdegremoval_amd import engine as E
    N, Cin, Cout, H, W, KH, st, pd = shape
    with arithmetic(mode, grad_scaled=scaled):
        runs = []
        for phase in range(SP.dgrad_phases(KH, st)):
            (dout, w), exp, mask = dgrad_case(shape, phase)
            dx, _, _ = E.conv_bwd(dev(dout), torch.zeros(N, Cin, H, W, device='cuda'), dev(w), st, pd)
            runs.append((dx, exp, mask))
        verdict(f'conv_bwd_dx_{KH}x{KH}s{st}', sid(shape) + ('-scaled' if scaled else ''), mode, cls, runs)


# ------------------------------------------------------------------ plane tensors: conv3x3_p16
def _p16_conv(K, shape, cfg, fmt):
    from textualdegremoval_amd import _lib
    N, Cin, Cout, H, W, *_ = shape
    (x, w), exp, mask = conv_case(shape)
    wp, mp, *_ = K.pack_weights(dev(w), K.PACK_FWD)
    x16 = K.p16_from_f32(dev(x), fmt=fmt)
    _lib.load().tdr_conv3x3_p16_force_cfg(cfg)
    try:
        o32, _ = K.conv3x3_p16(x16, wp, mp, Cout)
    finally:
        _lib.load().tdr_conv3x3_p16_force_cfg(0)
    return o32, exp, mask


@pytest.mark.parametrize('cfg', [0, 301, 302, 303, 304, 306, 307, 311, 321])
@pytest.mark.parametrize('shape', SP.P16_CONV_SHAPES, ids=sid)
def test_conv3x3_triple_planes(shape, cfg):
    with arithmetic('bx3') as K:
        verdict('conv3x3_p16_triple', f'cfg{cfg} {sid(shape)}', 'bx3', 'bx3', [_p16_conv(K, shape, cfg, K.FMT_BX3)])


@pytest.mark.parametrize('cfg', [0, 3, 16, 17, 19, 22])
@pytest.mark.parametrize('shape', SP.P16_CONV_SHAPES, ids=sid)
def test_conv3x3_pair_planes(shape, cfg):
    with arithmetic('hx2') as K:
        verdict('conv3x3_p16_pair', f'cfg{cfg} {sid(shape)}', 'hx2', 'hx2', [_p16_conv(K, shape, cfg, K.FMT_HX2)])


# ------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize('shape', SP.WGRAD_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', MODES)
def test_conv_wgrad(mode, shape):
    """fp16_range=True: under hx2 the 2-way fp16 split variant of the kernel is the one probed (as tests/test_hip_kernels.py does);
    stride 2: one launch per pixel parity (_split_probe.wgrad_phases)"""
    N, Cin, Cout, H, W, KH, st, pd, gate, per_image = shape
    with arithmetic(mode) as K:
        runs = []
        for phase in range(SP.wgrad_phases(st)):
            (x, dy), exp, mask = wgrad_case(shape, phase)
            g = K.conv_wgrad(dev(x), dev(dy), Cout, Cin, KH, stride=st, pad=pd, gate=gate, per_image=per_image, fp16_range=True)
            runs.append((g, exp, mask))
        verdict(f'conv_wgrad_{KH}x{KH}s{st}' + ('_gate' if gate else '') + ('_per_image' if per_image else ''), sid(shape[:8]), mode, mode, runs)


@pytest.mark.parametrize('shape', [s for s in SP.WGRAD_SHAPES if s[5] == 1], ids=sid)
@pytest.mark.parametrize('mode', MODES)
def test_conv_wgrad_1x1_exact_kernel(mode, shape):
    """kernels.WGRAD_1X1_BX3 off: the exact fp32 kernel whatever the mode -- pinned at the f32 bar"""
    N, Cin, Cout, H, W, KH, st, pd, gate, per_image = shape
    (x, dy), exp, mask = wgrad_case(shape)
    with arithmetic(mode, wgrad_1x1_bx3=False) as K:
        g = K.conv_wgrad(dev(x), dev(dy), Cout, Cin, 1, gate=gate, per_image=per_image, fp16_range=True)
        verdict('conv_wgrad_1x1_exact' + ('_gate' if gate else '') + ('_per_image' if per_image else ''), sid(shape[:8]), mode, 'f32', [(g, exp, mask)])


@pytest.mark.parametrize('mode,scaled,cls', DGRAD_MODES[:3])
def test_wgrad1x1_group(mode, scaled, cls):
    """three problems in one launch and one fixed-order reduction (exact fp32 has no grouped kernel)"""
    shape = SP.WGRAD_GROUP_SHAPE
    N, Cin, Cout, H, W, *_ = shape
    cases = [wgrad_case(shape, 0, seed) for seed in (7, 17, 27)]
    with arithmetic(mode, grad_scaled=scaled) as K:
        reqs = [(dev(x), dev(dy), Cout, Cin, False) for (x, dy), _, _ in cases]
        assert K.wgrad1x1_group_key(*reqs[0]) is not None
        assert len({K.wgrad1x1_group_key(*r) for r in reqs}) == 1
        out = K.wgrad1x1_group(reqs, seq=('split_probe', mode, scaled))
        verdict('wgrad1x1_group', 'x3 ' + sid(shape[:8]) + ('-scaled' if scaled else ''), mode, cls,
                [(g, exp, mask) for (g, _), (_, exp, mask) in zip(out, cases)])


@pytest.mark.parametrize('shape', SP.WGRAD_P16_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', ['bx3', 'hx2'])
def test_wgrad3x3_plane_tensors(mode, shape):
    """wgrad3x3_p16 and wgrad3x3_p16_group (two problems) on triple planes (bx3) and pair planes (hx2)"""
    cases = [wgrad_case(shape, 0, seed) for seed in (7, 17)]
    with arithmetic(mode) as K:
        fmt = K.FMT_BX3 if mode == 'bx3' else K.FMT_HX2
        planes = [(K.p16_from_f32(dev(x), fmt=fmt), K.p16_from_f32(dev(dy), fmt=fmt)) for (x, dy), _, _ in cases]
        g = K.wgrad3x3_p16(*planes[0])
        verdict('wgrad3x3_p16', sid(shape[:8]), mode, mode, [(g, cases[0][1], cases[0][2])])
        out = K.wgrad3x3_p16_group(planes, seq=('split_probe', shape, mode))
        verdict('wgrad3x3_p16_group', 'x2 ' + sid(shape[:8]), mode, mode, [(g, exp, mask) for (g, _), (_, exp, mask) in zip(out, cases)])


# ------------------------------------------------------------------ token-major GEMMs
def _tok(K, shape, split, gemm):
    P, N, Kd = shape
    runs = []
    for phase in range(SP.tok_phases(P, Kd)):
        (x, w), exp, mask = SP.build_tok(P, N, Kd, seed=9, phase=phase)
        runs.append((gemm(split(dev(x)), split(dev(w)), None, epi=3), exp, mask))
    return runs


@pytest.mark.parametrize('shape', SP.TOK3_SHAPES, ids=sid)
def test_tok16x3_gemm(shape):
    """64-row tiles of a short launch / 128-row tiles of a wide one, ragged last row tile; every k is some launch's"""
    with arithmetic('bx3') as K:
        verdict('tok16x3_gemm', sid(shape), 'bx3', 'bx3', _tok(K, shape, K.split_planes3, K.tok16x3_gemm))


@pytest.mark.parametrize('shape', SP.TOK2_SHAPES, ids=sid)
def test_tok16x2_gemm(shape):
    with arithmetic('hx2') as K:
        verdict('tok16x2_gemm', sid(shape), 'hx2', 'hx2', _tok(K, shape, K.split_planes, K.tok16x2_gemm))


# ------------------------------------------------------------------ the fused NAFBlock tail chain: its conv3 stage
@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', ['bx3', 'hx2'])
def test_chain_conv3_stage(mode, shape):
    """kernels.naf_tail_fwd with a one-hot gate output g, channel attention 1.0, beta 1.0, a zero conv3 bias and a zero block input: the
    saved tensor y = (W3 (g * sca) + b3) * beta + x is W3 g, one product per element.  HW = 64 * (C / 16) and N = 2: every value of the
    per-workgroup group rotation of gemm_split occurs.  conv4 / conv5 of the same launch, conv1 of the head chain and the backward chains:
    tests/test_hip_chain_probe.py."""
    N, C, H, W = shape
    (g, w3), exp, mask = conv_case((N, C, C, H, W, 1, 1, 0))
    r = lambda *s, seed: torch.randn(*s, generator=torch.Generator().manual_seed(seed)).cuda()
    with arithmetic(mode) as K:
        assert K.naf_tail_supported(C, H * W)
        w3p, w4p, w5p = (K.pack_weights(t, K.PACK_FWD)[0] for t in (dev(w3), r(2 * C, C, 1, 1, seed=1) * C ** -0.5, r(C, C, 1, 1, seed=2) * C ** -0.5))
        ones, zeros = torch.ones(C, device='cuda'), torch.zeros(C, device='cuda')
        out, y, *_ = K.naf_tail_fwd(dev(g), torch.ones(N, C, device='cuda'), torch.zeros(N, C, H, W, device='cuda'), w3p, zeros, ones,
                                    1.0 + 0.1 * r(C, seed=3), 0.1 * r(C, seed=4), 1e-6, w4p, 0.1 * r(2 * C, seed=5), w5p, 0.1 * r(C, seed=6),
                                    0.3 * r(C, seed=7))
        assert torch.isfinite(out).all()
        verdict('naf_tail_fwd_conv3', sid(shape), mode, mode, [(y, exp, mask)])
