"""The single-product probe without a GPU (tests/_split_probe.py): proof that its bars have teeth and that the reference
alone stays inside them.  Per scheme, on 2^20 sample pairs drawn like the probe's operands: the documented product list, emulated on the
CPU, stays under bar / 2; the same list with any ONE product removed exceeds 8 * bar (so a bar cannot be moved to within 8x of a wrong
kernel without this file failing).  Per builder and per shape that tests/test_hip_split_probe.py runs: `expected` equals a dense float64
convolution / einsum of the same inputs to 1e-15 relative, outputs outside the mask are exact zeros of that dense result, and at least
90 % of all outputs are single products (over the launches of a case where one launch cannot reach them all: stride-2 data and weight
gradients, K longer than the token count) -- the rest are the exact-zero border outputs.

The sample set is fixed.  For hx2 the maximum over 2^20 pairs depends on the draw: eight draws gave 4.5e-7 ... 4.9e-7 around bar / 2 =
4.77e-7 (this one: 4.56e-7), and the scheme's analytic worst case is the dropped mm term 2^-22 plus one rounding of each residual plane
2 * 2^-23 plus the last fp32 addition 2^-24 = 5.4e-7 = 0.56 bar -- reached only with both operands just above a power of two.  The
bar itself (2^-20) is 1.75x above that worst case and 500x below the smallest wrong variant; the bx3 maximum is 1.0e-7 in every draw."""
import pytest
import torch
import torch.nn.functional as F

import _split_probe as SP

NS = 1 << 20


@pytest.fixture(scope='module')
def samples():
    return SP.values(NS, seed=200), SP.values(NS, seed=300)


def _rel(got, a, b):
    ref = a.double() * b.double()
    return ((got.double() - ref).abs() / ref.abs())


@pytest.mark.parametrize('scheme', ['bx3', 'hx2', 'f32'])
def test_full_scheme_stays_under_half_the_bar(samples, scheme):
    a, b = samples
    worst = _rel(SP.emulate(a, b, scheme), a, b).max().item()
    print(f'emulated {scheme}: max rel {worst:.2e} (bar {SP.BAR[scheme]:.2e})')
    assert worst <= SP.BAR[scheme] / 2


@pytest.mark.parametrize('scheme,drop', [(s, d) for s in ('bx3', 'hx2') for d in SP.PRODUCTS[s]])
def test_every_dropped_product_exceeds_eight_bars(samples, scheme, drop):
    a, b = samples
    rel = _rel(SP.emulate(a, b, scheme, drop=drop), a, b)
    print(f'emulated {scheme} without {drop}: max rel {rel.max().item():.2e}, {100 * (rel > SP.BAR[scheme]).double().mean().item():.0f} % of the '
          f'samples over the bar {SP.BAR[scheme]:.2e}')
    assert rel.max().item() >= 8 * SP.BAR[scheme]


def test_planes_are_the_documented_splits(samples):
    a, _ = samples
    p3 = SP.split3_bf16(a)
    assert torch.equal((p3['h'] + p3['m']) + p3['l'], a)                      # 8 + 8 + 8 bits: the fp32 value
    for p in p3.values():
        assert torch.equal(p.bfloat16().float(), p)
    p2 = SP.split2_f16(a)
    assert ((p2['h'].double() + p2['m'].double() - a.double()).abs() <= 2.0 ** -22 * a.abs().double()).all()
    for p in p2.values():
        assert torch.equal(p.half().float(), p)


def _close(exp, dense, mask):
    assert exp.shape == dense.shape == mask.shape
    assert (dense[~mask] == 0).all() and (exp[~mask] == 0).all()
    assert (exp[mask] != 0).all()
    assert ((exp - dense).abs()[mask] / dense.abs()[mask]).max().item() <= 1e-15


FWD = [SP.CONV1X1_CFG_SHAPE, SP.CONV3X3_CFG_SHAPE, SP.GATE_SHAPE] + SP.CONV_FWD_SHAPES + SP.P16_CONV_SHAPES


@pytest.mark.parametrize('shape', FWD + [SP.CONV_PER_IMAGE_SHAPE], ids=lambda s: 'x'.join(map(str, s)))
def test_conv_builder_equals_dense_float64(shape):
    N, Cin, Cout, H, W, KH, st, pd = shape
    per_image = shape == SP.CONV_PER_IMAGE_SHAPE
    (x, w), exp, mask = SP.build_conv(*shape, seed=3, per_image=per_image)
    assert (x != 0).sum(1).max().item() == 1                                  # one-hot over the channels
    assert ((x != 0).sum((0, 2, 3)) > 0).all()                                # every channel is hit
    if per_image:
        dense = torch.cat([F.conv2d(x[n:n + 1].double(), w[n].double(), stride=st, padding=pd) for n in range(N)])
    else:
        dense = F.conv2d(x.double(), w.double(), stride=st, padding=pd)
    _close(exp, dense, mask)
    assert mask.double().mean().item() >= 0.9
    if KH > 1:                                                                # every tap is some output's
        taps = F.conv2d((x != 0).sum(1, keepdim=True).double(), torch.eye(KH * KH, dtype=torch.float64).view(KH * KH, 1, KH, KH), stride=st, padding=pd)
        assert (taps.sum((0, 2, 3)) > 0).all()


@pytest.mark.parametrize('shape', SP.DGRAD_SHAPES + [SP.GATE_SHAPE], ids=lambda s: 'x'.join(map(str, s)))
def test_dgrad_builder_equals_dense_float64(shape):
    N, Cin, Cout, H, W, KH, st, pd = shape
    masks = []
    for phase in range(SP.dgrad_phases(KH, st)):
        (dout, w), exp, mask = SP.build_dgrad(*shape, seed=5, phase=phase)
        assert (dout != 0).sum(1).max().item() == 1 and ((dout != 0).sum((0, 2, 3)) > 0).all()
        xz = torch.zeros(N, Cin, H, W, dtype=torch.float64, requires_grad=True)
        dense, = torch.autograd.grad(F.conv2d(xz, w.double(), stride=st, padding=pd), xz, dout.double())
        _close(exp, dense, mask)
        masks.append(mask)
    assert SP.coverage(masks) >= 0.9


@pytest.mark.parametrize('shape', SP.WGRAD_SHAPES + [SP.WGRAD_GROUP_SHAPE] + SP.WGRAD_P16_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_wgrad_builder_equals_dense_float64(shape):
    N, Cin, Cout, H, W, KH, st, pd, gate, per_image = shape
    masks = []
    for phase in range(SP.wgrad_phases(st)):
        (x, dy), exp, mask = SP.build_wgrad(N, Cin, Cout, H, W, KH, st, pd, seed=7, phase=phase, gate=gate, per_image=per_image)
        xe = (x[:, :Cin] * x[:, Cin:]) if gate else x
        assert torch.equal(xe, x[:, :Cin])
        per_ch = (xe != 0).sum((2, 3))                                        # [N, Cin]: one pixel per channel (per image with per_image)
        assert (per_ch == 1).all() if per_image else (per_ch.sum(0) == 1).all()
        dense = []
        for n in range(N):
            wz = torch.zeros(Cout, Cin, KH, KH, dtype=torch.float64, requires_grad=True)
            dense.append(torch.autograd.grad(F.conv2d(xe[n:n + 1].double(), wz, stride=st, padding=pd), wz, dy[n:n + 1].double())[0])
        dense = torch.stack(dense)
        if not per_image:
            # exact: every element has at most one non-zero term over the images
            assert ((dense != 0).sum(0) <= 1).all()
            dense = dense.sum(0, keepdim=True)
        _close(exp, dense, mask)
        masks.append(mask)
    assert SP.coverage(masks) >= 0.9


@pytest.mark.parametrize('shape', SP.TOK3_SHAPES + SP.TOK2_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_tok_builder_equals_dense_float64(shape):
    P, N, Kd = shape
    hit = torch.zeros(Kd, dtype=torch.bool)
    for phase in range(SP.tok_phases(P, Kd)):
        (x, w), exp, mask = SP.build_tok(P, N, Kd, seed=9, phase=phase)
        assert ((x != 0).sum(1) == 1).all() and mask.all()
        _close(exp, w.double() @ x.double().t(), mask)
        hit |= (x != 0).any(0)
    assert hit.all()                                                          # every k of the contraction is some launch's


@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_chain_layout_reaches_every_channel_in_every_workgroup_rotation(shape):
    N, C, H, W = shape
    assert H * W == 64 * (C // 16)
    (g, w), exp, mask = SP.build_conv(N, C, C, H, W, 1, seed=11)
    assert mask.all() and ((g != 0).sum((2, 3)) > 0).all()
    _close(exp, F.conv2d(g.double(), w.double()), mask)
