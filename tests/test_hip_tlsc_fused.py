"""The TLSC block (engine.naf_fwd_local, `NAFNetLocal`) on the fused forward-only chains: tdr_naf_head_infer, the depthwise stencil, the
box mean and tdr_naf_tail_infer_local, which forms the per-pixel channel attention from the box mean and walks conv3 .. conv5.
(1) the block against a float64 restatement, no further from it than the per-op launches it replaces; (2) the fused path is the one
taken where the shape allows and only there; (3) the whole network against the reference (tests/golden/make_golden_tlsc_w32.py);
(4) the walk keeps nothing; (5) it is not slower.  The float64 box mean of (1) is itself pinned against the reference's `AvgPool2d`
outputs in tests/golden/tlsc.npz (no GPU)."""
import gc
import os
import statistics

import numpy as np
import pytest
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
LN_EPS = 1e-6
# (c, (H, W), (k1, k2)), N = 2: a 64-pixel tile spans several image rows, the second image, a box that covers one axis only, every
# wave count of the chains (1, 2, 4, 8)
BLOCKS = [(32, (16, 24), (5, 7)), (64, (16, 16), (16, 3)), (128, (8, 16), (3, 16)), (256, (8, 8), (4, 5))]


def boxmean64(x, k1, k2):
    """TLSC box mean in the dtype of x: mean over k1 x k2 windows (clipped to the map), stride 1, replicate padding back to H x W with
    the smaller half in front (nafnet_local_arch.py:61-74)"""
    H, W = x.shape[-2:]
    out = F.avg_pool2d(x, (min(k1, H), min(k2, W)), stride=1)
    hv, wv = out.shape[-2:]
    return F.pad(out, ((W - wv) // 2, (W - wv + 1) // 2, (H - hv) // 2, (H - hv + 1) // 2), mode='replicate')


def test_float64_box_mean_is_the_reference_avgpool():
    """the yardstick's box mean against `AvgPool2d` of the reference (recorded float32 outputs; 2e-5 covers the cancellation error of
    the float32 integral image there, as in test_hip_tlsc.py)"""
    g = np.load(os.path.join(GOLDEN, 'tlsc.npz'))
    assert int(g['pool_n']) == 5
    for i in range(int(g['pool_n'])):
        x = torch.from_numpy(g[f'pool{i}_x']).double()
        k1, k2 = (int(v) for v in g[f'pool{i}_k'])
        got = boxmean64(x, k1, k2)
        assert got.shape == x.shape and (got - torch.from_numpy(g[f'pool{i}_out']).double()).abs().max().item() < 2e-5, i


def _ln64(x, w, b):
    mu = x.mean(1, keepdim=True)
    var = (x - mu).pow(2).mean(1, keepdim=True)
    return (x - mu) / (var + LN_EPS).sqrt() * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def block64(x, P, k1, k2):
    """the NAFBlock of network_nafnet_guided_arch.py:178-240 with its SCA pool replaced by the TLSC box mean, in float64 on the CPU"""
    x = x.double().cpu()
    P = {k: v.double().cpu() for k, v in P.items()}
    c = x.shape[1]
    t = F.conv2d(_ln64(x, P['norm1.weight'], P['norm1.bias']), P['conv1.weight'], P['conv1.bias'])
    t = F.conv2d(t, P['conv2.weight'], P['conv2.bias'], padding=1, groups=2 * c)
    g = t[:, :c] * t[:, c:]
    H, W = x.shape[-2:]
    pooled = g.mean((2, 3), keepdim=True) if k1 >= H and k2 >= W else boxmean64(g, k1, k2)
    s = F.conv2d(pooled, P['sca.1.weight'], P['sca.1.bias'])
    y = x + F.conv2d(g * s, P['conv3.weight'], P['conv3.bias']) * P['beta']
    t = F.conv2d(_ln64(y, P['norm2.weight'], P['norm2.bias']), P['conv4.weight'], P['conv4.bias'])
    return y + F.conv2d(t[:, :c] * t[:, c:], P['conv5.weight'], P['conv5.bias']) * P['gamma']


def _block_inputs(c, hw, seed, n=2):
    """random parameters as in test_hip_inference.py::test_forward_only_blocks_bitwise_and_switch"""
    gen = torch.Generator().manual_seed(seed)
    P = {}
    for nm, shp in [('beta', (1, c, 1, 1)), ('gamma', (1, c, 1, 1)), ('conv1.weight', (2 * c, c, 1, 1)), ('conv1.bias', (2 * c,)),
                    ('conv2.weight', (2 * c, 1, 3, 3)), ('conv2.bias', (2 * c,)), ('conv3.weight', (c, c, 1, 1)), ('conv3.bias', (c,)),
                    ('sca.1.weight', (c, c, 1, 1)), ('sca.1.bias', (c,)), ('conv4.weight', (2 * c, c, 1, 1)), ('conv4.bias', (2 * c,)),
                    ('conv5.weight', (c, c, 1, 1)), ('conv5.bias', (c,)), ('norm1.weight', (c,)), ('norm1.bias', (c,)),
                    ('norm2.weight', (c,)), ('norm2.bias', (c,))]:
        P[nm] = (torch.randn(shp, generator=gen) * 0.2 + (1.0 if nm in ('norm1.weight', 'norm2.weight') else 0.0)).cuda()
    return torch.randn(n, c, *hw, generator=gen).cuda(), P


@pytest.fixture
def set_math():
    from textualdegremoval_amd import kernels as K
    prev = K.MATH
    yield K.set_math
    K.set_math(prev)


def _local(x, P, k, on):
    from textualdegremoval_amd import engine as E
    prev, E.LOCAL_KERNELS = E.LOCAL_KERNELS, on
    try:
        return E.naf_fwd_local(x, P, *k)
    finally:
        E.LOCAL_KERNELS = prev


def _spy(monkeypatch, mod, name):
    """the calls of mod.<name>: their keyword arguments, in order"""
    orig, seen = getattr(mod, name), []

    def wrapped(*a, **k):
        seen.append(k)
        return orig(*a, **k)
    monkeypatch.setattr(mod, name, wrapped)
    return seen


def _rel(out, want):
    return ((out.double().cpu() - want).abs().max() / want.abs().max()).item()


@pytest.mark.gpu
@pytest.mark.parametrize('math', ['bx3', 'hx2'])
@pytest.mark.parametrize('c,hw,k', BLOCKS)
def test_fused_block_against_float64(set_math, monkeypatch, math, c, hw, k):
    """e = max|out - out64| / max|out64| of the fused block and of the per-op launches (the code before the fused path, the yardstick):
    e_fused <= max(4 e_perop, 2e-6) and <= 1e-4, the project's parity bar.  4 x: another summation order of the same arithmetic class,
    over a maximum of a few thousand samples."""
    from textualdegremoval_amd import kernels as K
    set_math(math)
    x, P = _block_inputs(c, hw, 100 + c)
    want = block64(x, P, *k)
    calls = _spy(monkeypatch, K, 'naf_tail_infer_local')
    fused = _local(x, P, k, True)
    assert len(calls) == 1
    perop = _local(x, P, k, False)
    assert len(calls) == 1
    e_fused, e_perop = _rel(fused, want), _rel(perop, want)
    print(f'TLSC block c={c} {hw[0]}x{hw[1]} box {k} {math}: e_fused {e_fused:.3e} e_perop {e_perop:.3e}')
    assert e_fused <= max(4 * e_perop, 2e-6) and e_fused <= 1e-4, (e_fused, e_perop)


@pytest.mark.gpu
def test_fused_path_is_taken_where_the_shape_allows_and_only_there(set_math, monkeypatch):
    from textualdegremoval_amd import engine as E, kernels as K
    set_math('bx3')
    tail, head, copy, ln = (_spy(monkeypatch, K, n) for n in ('naf_tail_infer_local', 'naf_head_infer', 'copy_rows', 'layernorm2d_fwd'))
    x, P = _block_inputs(64, (16, 16), 7)
    out = _local(x, P, (5, 5), True)
    assert (len(tail), len(head), len(copy), len(ln)) == (1, 1, 0, 0)
    assert _rel(out, block64(x, P, 5, 5)) <= 1e-4
    # the ways to the per-op launches: the switch, a channel count and a pixel count the chains do not take, the fp32 arithmetic
    for what, c, hw, on, math in (('switch', 64, (16, 16), False, 'bx3'), ('c = 48', 48, (16, 16), True, 'bx3'),
                                  ('HW % 64', 64, (12, 8), True, 'bx3'), ('f32', 64, (16, 16), True, 'f32')):
        set_math(math)
        x, P = _block_inputs(c, hw, 8)
        out = _local(x, P, (5, 5), on)
        assert len(tail) == 1 and len(copy) >= 1 and len(ln) >= 2, what
        assert _rel(out, block64(x, P, 5, 5)) <= 1e-4, what
        del copy[:], ln[:]
    # a box that covers the whole map: the ordinary block as a pass that keeps nothing -- the bits of the training forward
    set_math('bx3')
    x, P = _block_inputs(64, (16, 16), 9)
    want = E.naf_fwd(x, P)[0]
    fwd = _spy(monkeypatch, E, 'naf_fwd')
    out = _local(x, P, (16, 24), True)
    assert fwd == [{'keep': False}] and len(tail) == 1
    assert torch.equal(out, want)


def _golden_net():
    from textualdegremoval_amd.models.archs import define_network
    g = np.load(os.path.join(GOLDEN, 'tlsc_w32.npz'))
    net = define_network(dict(type='NAFNetLocal', img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=[1], dec_blk_nums=[1],
                              train_size=(1, 3, 32, 32)))
    return g, net


@pytest.mark.gpu
@pytest.mark.parametrize('math', ['bx3', 'hx2'])
def test_nafnet_local_w32_vs_reference(set_math, monkeypatch, math):
    """width 32, one encoder level, 63 x 95 padded to 64 x 96: 32 channels at HW 6144 under a 48 x 48 box (encoder, decoder), 64 at HW 1536
    under 24 x 24 (middle) -- every block takes the chain and pools locally"""
    from textualdegremoval_amd import kernels as K
    set_math(math)
    g, net = _golden_net()
    assert [k for k, _ in net.named_parameters()] == [str(k) for k in g['names']]
    net.load_state_dict({str(k): torch.from_numpy(g['p_' + str(k)]) for k in g['names']}, strict=True)
    net = net.cuda()
    ks = [tuple(int(v) for v in k) for k in g['ksizes']]           # modules() order: encoder, decoder (both level 0), middle
    assert net.ksizes == [ks[0], ks[2]] and ks[1] == ks[0]
    tail = _spy(monkeypatch, K, 'naf_tail_infer_local')
    out = net(torch.from_numpy(g['x']).cuda())
    assert not out.requires_grad and len(tail) == 3
    err = (out.cpu() - torch.from_numpy(g['out'])).abs().max().item()
    print(f'NAFNetLocal width 32 {math}: max|out - reference| {err:.3e}')
    assert err < 1e-4


def _deep_net():
    """width 32, enc [1, 1, 1, 4]: 32 .. 256 channels on the chains (the 512 of the middle on the per-op launches either way); at 256 x 256
    every level is larger than its box (1.5 x 128 >> level)"""
    from textualdegremoval_amd.models.archs import define_network
    net = define_network(dict(type='NAFNetLocal', img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 4],
                              dec_blk_nums=[1, 1, 1, 1], train_size=(1, 3, 128, 128)))
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if k.endswith(('beta', 'gamma')):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
    return net.cuda(), torch.rand(1, 3, 256, 256, generator=gen).cuda()


def _switched(net, x, on, rep=1):
    from textualdegremoval_amd import engine as E
    prev, E.LOCAL_KERNELS = E.LOCAL_KERNELS, on
    try:
        for _ in range(rep):
            out = net(x)
        return out
    finally:
        E.LOCAL_KERNELS = prev


def _peak_delta(fn):
    """torch.cuda.max_memory_allocated() above what was allocated before fn() ran, fn's result still alive at the end (as in
    test_hip_inference.py)"""
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


@pytest.mark.gpu
def test_nothing_kept_peak_memory_no_higher_than_per_op():
    """both paths walk with keep=False and hold the same skips; on top of them a fused block has 4 c-planes of working set at level 0
    (x, g, box mean, out; or x, t1, g), the per-op block about 12 (x, g, the concatenation, y, yn, t4, out).  Measured in alternation
    after one warm-up call of each (workspaces, code objects)."""
    net, x = _deep_net()
    for on in (True, False):
        _switched(net, x, on)
    peaks = {True: [], False: []}
    for _ in range(2):
        for on in (True, False):
            peaks[on].append(_peak_delta(lambda: _switched(net, x, on)))
    print('NAFNetLocal 1x3x256x256 width 32, peak memory above the resident state: fused ' +
          ' / '.join(f'{p / 2**20:.1f}' for p in peaks[True]) + ' MiB, per-op ' + ' / '.join(f'{p / 2**20:.1f}' for p in peaks[False]) + ' MiB')
    assert all(p_on <= p_off for p_on, p_off in zip(peaks[True], peaks[False])), peaks


@pytest.mark.gpu
def test_fused_forward_is_not_slower_than_per_op():
    """same process, same shape, alternating runs, medians of device time over 11 rounds (two events around three forwards), after
    warm-up: the scheme of test_hip_inference.py::test_no_grad_forward_is_not_slower"""
    net, x = _deep_net()
    REP = 3

    def timed(on):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        _switched(net, x, on, REP)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REP
    for on in (False, True, False, True):
        timed(on)
    t_off, t_on = [], []
    for _ in range(11):
        t_off.append(timed(False))
        t_on.append(timed(True))
    m_off, m_on = statistics.median(t_off), statistics.median(t_on)
    print(f'NAFNetLocal forward at 1x3x256x256, width 32: per-op median {m_off:.2f} ms (min {min(t_off):.2f}), fused median {m_on:.2f} ms '
          f'(min {min(t_on):.2f})')
    assert m_on <= m_off, (t_on, t_off)
