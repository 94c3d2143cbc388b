"""The float4-staged 1x1 kernel, conv1x1_staged_kernel (csrc/tdr_conv_bx3.hip), of every arithmetic (bx3, hx2, h1) against the generic
conv_bx3_kernel it replaces on eligible launches.  The two differ in how the pixels reach the LDS planes and in nothing else -- same
weight fragments, same products per 16-channel group in the same order (six, three, one), same accumulators and epilogues -- so every
case asserts BIT equality (torch.equal) between the launch with kernels.CONV1X1_STAGED on and the same launch with it off.  Before that
each case asks the library (kernels.conv1x1_staged_takes -> tdr_conv1x1_bx3_staged_takes) whether the launch is routed to the staged
kernel, so no case can pass by comparing the generic kernel with itself, and the decline cases assert the opposite.  One eligible shape
of bx3 and one of hx2 are also pinned on their own against float64 with the single-product probe (tests/_split_probe.py): six products,
bar 2^-21; three products, bar 2^-20.

Every tile configuration the heuristic can pick has its own case (test_every_tile_configuration, test_hx2_every_tile_configuration): a
forced configuration stays on the generic kernel, so the tile is chosen by the shape -- stage length, octets per stage and quads per tile
differ between them (bx3: 32 channels of 128 pixels, 64 of 64, 16 of 256; hx2 / h1: twice that).

Shapes: the smallest at which the staging can go wrong.  bx3: a 128-pixel tile stages 32 channels at a time (half an octet x four pixels
per thread), so Cin = 200 has a partial octet, a partial 16-channel group and a partial last stage; 12 x 12 pixels leave quads wholly
outside a tile; Cin = 96 is one stage short of the four the dispatch asks for.  hx2 / h1: a 128-pixel tile stages 64 channels (an octet
x four pixels per thread), so four stages need Cin >= 193: Cin = 200 again has the partial octet, group and last stage, Cin = 192 is one
stage short, and a launch of more than 512 workgroups stays on the generic kernel.

The fixture K sets the arithmetic: bx3 unless a case asks for another (@MATH('hx2'))."""
import pytest
import torch

import _split_probe as SP

pytestmark = pytest.mark.gpu


@pytest.fixture
def K(request):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels
    prev_math, prev_switch = kernels.MATH, kernels.CONV1X1_STAGED
    kernels.set_math(getattr(request, 'param', 'bx3'))
    kernels.CONV1X1_STAGED = True
    try:
        yield kernels
    finally:
        kernels.set_math(prev_math)
        kernels.CONV1X1_STAGED = prev_switch


def MATH(mode):
    return pytest.mark.parametrize('K', [mode], indirect=True)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def both(K, staged, x, wp, mp, Cout, make_out=None, view=lambda o: o, **kw):
    """the launch with the switch on and off -> the staged kernel's output; asserts the routing first, bit equality after"""
    outs = []
    for on in (True, False):
        K.CONV1X1_STAGED = on
        buf = make_out() if make_out is not None else None
        extra = dict(kw, out=view(buf)) if buf is not None else kw
        takes = K.conv1x1_staged_takes(x, wp, mp, Cout, 1, **extra)
        assert takes == (staged and on), f'switch {on}: the query says {takes}'
        out = K.conv_forward(x, wp, mp, Cout, 1, **extra)
        outs.append(buf if buf is not None else out)
    K.CONV1X1_STAGED = True
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0]).all()
    assert torch.equal(outs[0], outs[1]), f'max |staged - generic| = {(outs[0] - outs[1]).abs().max().item():.3e}'
    return outs[0]


def fwd_pack(K, Cout, Cin, seed):
    wp, mp, *_ = K.pack_weights(rnd(Cout, Cin, 1, 1, seed=seed, scale=0.1), K.PACK_FWD)
    return wp, mp


def test_ragged_k(K):
    """N = 2, 200 -> 96, 8 x 16: partial octet, partial group, partial last stage; the last m-tile is clamped; one 128-pixel tile"""
    wp, mp = fwd_pack(K, 96, 200, seed=1)
    both(K, True, rnd(2, 200, 8, 16, seed=2), wp, mp, 96)


def test_ragged_pixels_odd_batch(K):
    """N = 3, 136 -> 160, 12 x 12: a partial second pixel tile, quads wholly inside or outside, a grid that is no multiple of 8"""
    wp, mp = fwd_pack(K, 160, 136, seed=3)
    both(K, True, rnd(3, 136, 12, 12, seed=4), wp, mp, 160)


# N, Cin, Cout, H, W -> the tile launch_bx_shape picks (co x pixels), its stage length; the smallest batch / image that makes the heuristic pick it
TILE_CASES = {
    '128x128': (4, 256, 512, 64, 64),      # Cout > 64 and 512 blocks of 128 x 128: 32-channel stages
    '256x64': (4, 1003, 1024, 32, 32),     # Cin >= 768, Cout >= 256, 256 blocks of 256 x 64: 64-channel stages, ragged Cin (partial octet, group and stage)
    '32x256': (8, 52, 32, 128, 128),       # Cout <= 32 and 512 blocks of 32 x 256: 16-channel stages, four of them, ragged Cin
    '32x128': (2, 100, 24, 16, 16),        # Cout <= 32, fewer blocks: 32-channel stages, ragged Cin
    '64x256': (8, 72, 48, 128, 128),       # Cout <= 64 and 512 blocks of 64 x 256: 16-channel stages, ragged Cin, rows past Cout
    '64x128': (2, 200, 96, 8, 16),         # (the tile of every other case of this file)
}


@pytest.mark.parametrize('tile', list(TILE_CASES))
def test_every_tile_configuration(K, tile):
    N, Cin, Cout, H, W = TILE_CASES[tile]
    wp, mp = fwd_pack(K, Cout, Cin, seed=31)
    both(K, True, rnd(N, Cin, H, W, seed=32), wp, mp, Cout, bias=rnd(Cout, seed=33))


def test_gate_and_kscale(K):
    """the operand x[:, :144] * x[:, 144:] * kscale[n, c], formed while staging"""
    wp, mp = fwd_pack(K, 72, 144, seed=5)
    both(K, True, rnd(2, 288, 8, 16, seed=6), wp, mp, 72, gate=True, kscale=rnd(2, 144, seed=7))


@pytest.mark.parametrize('with_mask', [False, True])
def test_std_epilogue_fields_together(K, with_mask):
    N, Cin, Cout, H, W = 2, 136, 96, 8, 16
    wp, mp = fwd_pack(K, Cout, Cin, seed=8)
    kw = dict(bias=rnd(Cout, seed=9), scale=rnd(Cout, seed=10), bias2=rnd(N, Cout, seed=11), bias2_mul=0.75,
              res=rnd(N, Cout, H, W, seed=12), relu=1)
    if with_mask:
        kw['mask'] = (rnd(N, Cout, H, W, seed=13) > 0).float()
    out = both(K, True, rnd(N, Cin, H, W, seed=14), wp, mp, Cout, **kw)
    assert (out >= 0).all() and (out == 0).any()                    # the relu ran


def test_gatebwd_epilogue(K):
    """EPI_GATEBWD as engine.naf_bwd calls it: a PACK_DGRAD_S1 pack, kscale = gamma, aux = t4"""
    N, C, Cd, H, W = 2, 64, 128, 8, 16                              # dout [N, Cd] -> u [N, C] -> dt4 [N, 2 C]
    wp, mp, *_ = K.pack_weights(rnd(Cd, C, 1, 1, seed=15, scale=0.1), K.PACK_DGRAD_S1)
    out = both(K, True, rnd(N, Cd, H, W, seed=16), wp, mp, C, epi=K.EPI_GATEBWD, kscale=rnd(Cd, seed=17),
               aux=rnd(N, 2 * C, H, W, seed=18))
    assert tuple(out.shape) == (N, 2 * C, H, W)


def test_strided_views(K):
    """input: a channel slice of a wider tensor (in_ns > Cin HW); output: a slice of a concatenation buffer (out_ns > Cout HW)"""
    N, Cin, Cout, H, W = 2, 136, 96, 8, 16
    wp, mp = fwd_pack(K, Cout, Cin, seed=19)
    wide = rnd(N, Cin + 24, H, W, seed=20)
    out = both(K, True, wide[:, 8:8 + Cin], wp, mp, Cout, make_out=lambda: torch.full((N, Cout + 48, H, W), 7.0, device='cuda'),
               view=lambda o: o[:, 16:16 + Cout])
    assert (out[:, :16] == 7.0).all() and (out[:, 16 + Cout:] == 7.0).all() and (out[:, 16:16 + Cout] != 7.0).any()


def test_per_image_weights(K):
    """tdr_pack_weights_bx3_batch packs, wp_ns != 0: image n contracts with its own matrix"""
    N, Cin, Cout, H, W = 3, 136, 64, 8, 16
    wp, per = K.pack_f32packed_to_bx3(rnd(N, Cin, Cout, seed=21, scale=0.1))
    both(K, True, rnd(N, Cin, H, W, seed=22), wp, Cout, Cout, wp_ns=per)


def test_data_gradient_pack(K):
    """256 -> 128 as a data gradient (PACK_DGRAD_S1 of a 128 -> 256 convolution's weights)"""
    wp, mp, *_ = K.pack_weights(rnd(256, 128, 1, 1, seed=23, scale=0.1), K.PACK_DGRAD_S1)
    both(K, True, rnd(2, 256, 16, 16, seed=24, scale=1e-4), wp, mp, 128)


def test_declined_launches_stay_on_the_generic_kernel(K):
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    wp, mp = fwd_pack(K, 96, 136, seed=25)
    both(K, False, rnd(2, 136, 8, 10, seed=26), wp, mp, 96)         # W = 10: no aligned pixel quads
    wp, mp = fwd_pack(K, 96, 96, seed=27)
    both(K, False, rnd(2, 96, 8, 16, seed=28), wp, mp, 96)          # three 32-channel stages: one short of four
    wp, mp = fwd_pack(K, 96, 200, seed=1)
    x = rnd(2, 200, 8, 16, seed=2)
    assert K.conv1x1_staged_takes(x, wp, mp, 96, 1)
    lib.tdr_conv_force_cfg(1, 3)                                    # a forced tile configuration names the generic kernel
    try:
        both(K, False, x, wp, mp, 96)
    finally:
        lib.tdr_conv_force_cfg(1, 0)
    assert K.conv1x1_staged_takes(x, wp, mp, 96, 1)


def test_single_product_probe_against_float64(K):
    """one-hot operands: every output is ONE product a * b, so the staged kernel's own product list is pinned at the bx3 bar"""
    N, Cin, Cout, H, W = 2, 200, 96, 16, 16
    (x, w), exp, mask = SP.build_conv(N, Cin, Cout, H, W, 1, seed=3)
    wp, mp, *_ = K.pack_weights(w.cuda().contiguous(), K.PACK_FWD)
    xd = x.cuda().contiguous()
    assert K.conv1x1_staged_takes(xd, wp, mp, Cout, 1)
    out = K.conv_forward(xd, wp, mp, Cout, 1)
    assert tuple(out.shape) == tuple(exp.shape)
    assert SP.zeros_exact(out, mask), 'an output without a non-zero term is not exactly 0.0'
    worst = SP.max_rel(out, exp, mask)
    print(f'probe conv1x1_staged {N}x{Cin}x{Cout}x{H}x{W} bx3: max rel {worst:.2e} (bar {SP.BAR["bx3"]:.2e})')
    assert worst <= SP.BAR['bx3'], (worst, SP.BAR['bx3'])


# ---- hx2 / h1: the same kernel with whole-octet tasks, 64-channel stages at a 128-pixel tile, two planes / one

@MATH('hx2')
def test_hx2_ragged_k(K):
    """N = 2, 200 -> 96, 8 x 16: four 64-channel stages with a partial last one, a partial octet, a partial group; one 128-pixel tile"""
    wp, mp = fwd_pack(K, 96, 200, seed=41)
    both(K, True, rnd(2, 200, 8, 16, seed=42), wp, mp, 96)


@MATH('hx2')
def test_hx2_ragged_pixels_odd_batch(K):
    """N = 3, 264 -> 160, 12 x 12: five stages, a partial second pixel tile, quads wholly inside or outside, a grid that is no multiple of 8"""
    wp, mp = fwd_pack(K, 160, 264, seed=43)
    both(K, True, rnd(3, 264, 12, 12, seed=44), wp, mp, 160)


@MATH('hx2')
def test_hx2_gate_and_kscale(K):
    """the operand x[:, :200] * x[:, 200:] * kscale[n, c], formed while staging: the gated kernel has ONE register set of operand loads"""
    wp, mp = fwd_pack(K, 72, 200, seed=45)
    both(K, True, rnd(2, 400, 8, 16, seed=46), wp, mp, 72, gate=True, kscale=rnd(2, 200, seed=47))


# N, Cin, Cout, H, W as TILE_CASES; hx2 stages are twice as long, so Cin is the smallest ragged one with four of them
HX2_TILE_CASES = {
    '128x128': (4, 256, 512, 64, 64),      # 64-channel stages; exactly the 512 workgroups of the cap
    '256x64': (4, 1003, 1024, 32, 32),     # 128-channel stages, eight of them, ragged Cin
    '32x256': (8, 100, 32, 128, 128),      # 32-channel stages, four of them, ragged Cin; 512 workgroups
    '32x128': (2, 200, 24, 16, 16),        # 64-channel stages
    '64x256': (8, 100, 48, 128, 128),      # 32-channel stages, rows past Cout; 512 workgroups
    '64x128': (2, 200, 96, 8, 16),
}


@MATH('hx2')
@pytest.mark.parametrize('tile', list(HX2_TILE_CASES))
def test_hx2_every_tile_configuration(K, tile):
    N, Cin, Cout, H, W = HX2_TILE_CASES[tile]
    wp, mp = fwd_pack(K, Cout, Cin, seed=51)
    both(K, True, rnd(N, Cin, H, W, seed=52), wp, mp, Cout, bias=rnd(Cout, seed=53))


@MATH('hx2')
def test_hx2_declined_launches_stay_on_the_generic_kernel(K):
    wp, mp = fwd_pack(K, 96, 264, seed=55)
    both(K, False, rnd(2, 264, 8, 10, seed=56), wp, mp, 96)         # W = 10: no aligned pixel quads
    wp, mp = fwd_pack(K, 96, 192, seed=57)
    both(K, False, rnd(2, 192, 8, 16, seed=58), wp, mp, 96)         # three 64-channel stages: one short of four
    wp, mp = fwd_pack(K, 512, 256, seed=59)
    both(K, False, rnd(5, 256, 64, 64, seed=60), wp, mp, 512)       # 640 workgroups of 128 x 128: over the cap of 512 (N = 4 is taken, above)


@MATH('h1')
def test_h1_ragged_k(K):
    """the one-plane form of the same kernel (an hx2 pack's head plane, one product): N = 2, 200 -> 96, 8 x 16"""
    wp, mp = fwd_pack(K, 96, 200, seed=61)
    both(K, True, rnd(2, 200, 8, 16, seed=62), wp, mp, 96)


@MATH('hx2')
def test_hx2_single_product_probe_against_float64(K):
    """one-hot operands: every output is ONE product a * b, so the staged kernel's own product list is pinned at the hx2 bar"""
    N, Cin, Cout, H, W = 2, 200, 96, 16, 16
    (x, w), exp, mask = SP.build_conv(N, Cin, Cout, H, W, 1, seed=3)
    wp, mp, *_ = K.pack_weights(w.cuda().contiguous(), K.PACK_FWD)
    xd = x.cuda().contiguous()
    assert K.conv1x1_staged_takes(xd, wp, mp, Cout, 1)
    out = K.conv_forward(xd, wp, mp, Cout, 1)
    assert tuple(out.shape) == tuple(exp.shape)
    assert SP.zeros_exact(out, mask), 'an output without a non-zero term is not exactly 0.0'
    worst = SP.max_rel(out, exp, mask)
    print(f'probe conv1x1_staged {N}x{Cin}x{Cout}x{H}x{W} hx2: max rel {worst:.2e} (bar {SP.BAR["hx2"]:.2e})')
    assert worst <= SP.BAR['hx2'], (worst, SP.BAR['hx2'])
