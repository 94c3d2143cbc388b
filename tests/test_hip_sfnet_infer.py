"""GPU checks of SFNet's forward-only route: the fused GELU -> Gap / Patch_ap pair (tdr_sf_act_region_sums / _apply) against a float64
reference with the per-op composition's own error as the yardstick, tdr_sf_dynfilt_fwd without a `low` plane, and the whole network --
keep=False with the per-op kernels bit-equal to the eval pass on the training walk, the fused walk against the reference goldens
(tests/golden/sfnet_eval.npz) and the float64 oracle, buffers untouched, less memory, the nn.Module after .eval(), TLSC."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sfnet_oracle as SO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'sfnet_eval.npz')


@pytest.fixture(scope='module')
def KK():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels
    return kernels


@pytest.fixture(scope='module', params=['bx3', 'f32'])
def K(request, KK):
    prev = KK.MATH
    KK.set_math(request.param)
    yield KK
    KK.set_math(prev)


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def md(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def ulp32(v):
    """one float32 ulp at magnitude v"""
    return float(np.spacing(np.float32(v)))


class fused_kernels:
    """sfnet_engine.INFER_KERNELS for the duration of a block"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from textualdegremoval_amd import sfnet_engine as SE
        self.prev, SE.INFER_KERNELS = SE.INFER_KERNELS, self.on

    def __exit__(self, *exc):
        from textualdegremoval_amd import sfnet_engine as SE
        SE.INFER_KERNELS = self.prev
        return False


# ---------------------------------------------------------------------------------------------------------------- the kernel pair
@pytest.mark.parametrize('act', [1, 0])
@pytest.mark.parametrize('shape,rows', [((3, 12, 8, 12), None),       # 4 x 6 quadrants: scalar path, one chunk
                                        ((2, 8, 16, 24), 3),          # 8 x 12 quadrants: float4 path, chunks of 3, 3 and 2 rows
                                        ((1, 4, 64, 80), None),       # 32 x 40 quadrants
                                        ((520, 128, 4, 4), None)])    # N * C = 66560 planes: past the 65535 of a grid's y / z
def test_act_region_affine_against_float64(KK, shape, rows, act):
    """fused pair vs F.gelu + oracle.region_affine in double on each half; tolerance = what the per-op composition (K.gelu_fwd, then
    K.region_affine_fwd on each half) itself leaves against the same reference: err_fused <= 2 err_parent + 1 ulp (another summation
    order of the same length).  NaN-prefilled output and partials: an element nobody wrote shows; two runs are bit-equal."""
    N, C, H, W = shape
    h = C // 2
    z = rnd(N, C, H, W, seed=101)
    gh, gd = rnd(h, seed=102, scale=0.5), rnd(h, seed=103, scale=0.5)
    ph, pl = rnd(4 * h, seed=104, scale=0.5), rnd(4 * h, seed=105, scale=0.5)
    v = F.gelu(z.double()) if act else z.double()
    ref = torch.cat([SO.region_affine(v[:, :h], gh.double() + 1.0, gd.double() - gh.double() - 1.0, 1),
                     SO.region_affine(v[:, h:], ph.double(), pl.double() - ph.double(), 2)], 1)
    zc, ghc, gdc, phc, plc = (t.cuda() for t in (z, gh, gd, ph, pl))
    rows_used, chunks = KK.sf_region_chunks(H, W, rows)
    if rows is not None:
        assert (rows_used, chunks) == (3, 3)
    runs = []
    for _ in range(2):
        out = torch.full((N, C, H, W), float('nan'), device='cuda')
        part = torch.full((N * C * 4 * chunks,), float('nan'), device='cuda')
        got = KK.sf_act_region_affine(zc, ghc, gdc, phc, plc, act, out=out, rows_per_chunk=rows, part=part)
        assert got is out and not torch.isnan(out).any() and not torch.isnan(part).any()
        runs.append(out)
    assert torch.equal(runs[0], runs[1]) and torch.equal(zc.cpu(), z)                # deterministic; the input is left alone
    y = KK.gelu_fwd(zc)[1] if act else zc
    par = torch.empty_like(zc)
    KK.region_affine_fwd(y[:, :h], ghc, gdc, 1.0, 1, par[:, :h])
    KK.region_affine_fwd(y[:, h:], phc, plc, 0.0, 2, par[:, h:])
    err_fused, err_parent, ulp = md(runs[0], ref), md(par, ref), ulp32(ref.abs().max().item())
    print(f'act_region_affine {shape} rows {rows} act {act}: err fused {err_fused:.3e}  per-op {err_parent:.3e}  ulp {ulp:.3e}')
    assert err_fused <= 2 * err_parent + ulp, (err_fused, err_parent, ulp)
    # in place over z (what the walk does): the same bits
    zz = zc.clone()
    assert KK.sf_act_region_affine(zz, ghc, gdc, phc, plc, act, out=zz, rows_per_chunk=rows) is zz and torch.equal(zz, runs[0])


@pytest.mark.parametrize('k', [3, 5])
def test_dynfilt_without_a_low_plane_writes_the_same_mix(KK, k):
    N, c, H, W, G = 2, 16, 12, 20, 8
    big = rnd(N, 2 * c, H, W, seed=111).cuda()                                       # a channel slice, as the ResBlock passes it
    taps = torch.softmax(rnd(N, G, k * k, seed=112), -1).reshape(N, G * k * k).cuda()
    att = torch.softmax(rnd(N, 2 * c, seed=113), -1)
    ah, al = att[:, :c].contiguous().cuda(), att[:, c:].contiguous().cuda()
    low, mix = KK.sf_dynfilt_fwd(big[:, c:], taps, ah, al, k, G)
    none, mix2 = KK.sf_dynfilt_fwd(big[:, c:], taps, ah, al, k, G, want_low=False)
    assert none is None and low is not None and torch.equal(mix, mix2) and float(mix.abs().max()) > 0


def test_gelu_in_place_has_the_bits_of_gelu_fwd(KK):
    x, b = rnd(2, 5, 12, 20, seed=121).cuda(), rnd(5, seed=122).cuda()
    for bias in (None, b):
        y = KK.gelu_fwd(x, bias=bias)[1]
        t = x.clone()
        assert KK.gelu_(t, bias=bias) is t and torch.equal(t, y)


# ---------------------------------------------------------------------------------------------------------------- the whole network
_oracle64 = {}


def oracle64(tag, sd, x, num_res):
    """sfnet_forward after .eval() in float64 on the CPU, once per tag"""
    if tag not in _oracle64:
        P = {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}
        with torch.no_grad():
            _oracle64[tag] = [o.clone() for o in SO.sfnet_forward(P, x.double(), num_res, training=False)]
    return _oracle64[tag]


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    return out, torch.cuda.max_memory_allocated() - base


@pytest.mark.parametrize('tag', ['eval_r2', 'eval_r1_one'])
def test_forward_only_walk_against_the_eval_pass_the_golden_and_float64(K, tag):
    from textualdegremoval_amd import sfnet_engine as SE
    from textualdegremoval_amd.models.archs import define_network
    ge = np.load(GOLDEN, allow_pickle=False)
    num_res, seed, n, h, w = (int(v) for v in ge[tag + '_cfg'])
    sd = SO.synth_state(num_res, seed)
    P = {k: v.clone().cuda() for k, v in sd.items()}
    xh = torch.from_numpy(ge[tag + '_x'])
    x = xh.cuda()
    SE.net_fwd(P, x, num_res, training=False, keep=False)                            # (warm-up: workspaces and tables exist before the peaks)
    (kept, saved), peak_keep = peak_of(lambda: SE.net_fwd(P, x, num_res, training=False, keep=True))
    assert saved is not None
    del saved
    with fused_kernels(False):
        (perop, none), peak_perop = peak_of(lambda: SE.net_fwd(P, x, num_res, training=False, keep=False))
    assert none is None and all(torch.equal(a, b) for a, b in zip(kept, perop))      # the parent's path, bit for bit
    with fused_kernels(True):
        (fused, none), peak_fused = peak_of(lambda: SE.net_fwd(P, x, num_res, training=False, keep=False))
        again = SE.net_fwd(P, x, num_res, training=False)[0]                         # keep defaults to `training`
    assert none is None and all(torch.equal(a, b) for a, b in zip(fused, again))
    ref = oracle64(tag, sd, xh, num_res)
    for i, o in enumerate(fused):
        want = torch.from_numpy(ge[f'{tag}_out{i}'])
        assert o.shape == want.shape and md(o, want) < 1e-4, (i, md(o, want))
        err_fused, err_perop, ulp = md(o, ref[i]), md(perop[i], ref[i]), ulp32(ref[i].abs().max().item())
        print(f'{tag} [{K.MATH}] out{i}: err fused {err_fused:.3e}  per-op {err_perop:.3e}  ulp {ulp:.3e}')
        assert err_fused <= 2 * err_perop + ulp, (i, err_fused, err_perop, ulp)
    assert all(torch.equal(P[k].cpu(), sd[k]) for k in sd if SO.is_buffer(k))        # BatchNorm buffers untouched
    print(f'{tag} [{K.MATH}]: peak above resident  keep=True {peak_keep}  keep=False per-op {peak_perop}  fused {peak_fused}')
    assert peak_fused < peak_keep and peak_perop < peak_keep
    net = define_network(dict(type='SFNet', mode=['train', 'Indoor'], num_res=num_res)).cuda()
    net.load_state_dict(sd)
    net.eval()
    for ctx in (torch.no_grad(), torch.enable_grad()):                               # selected by .eval() alone, whatever the grad mode
        with ctx:
            mo = net(x)
        assert all(torch.equal(a, b) and not a.requires_grad for a, b in zip(mo, fused))
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in net.state_dict().items())


def test_forward_only_walk_with_tlsc_pooling_against_the_golden(K):
    from textualdegremoval_amd import sfnet_engine as SE
    tag = 'test_indoor_r2'
    ge = np.load(GOLDEN, allow_pickle=False)
    num_res, seed, n, h, w = (int(v) for v in ge[tag + '_cfg'])
    sd = SO.synth_state(num_res, seed)
    P = {k: v.clone().cuda() for k, v in sd.items()}
    x = torch.from_numpy(ge[tag + '_x']).cuda()
    outs, none = SE.net_fwd(P, x, num_res, training=False, tlsc=SE.TLSC_BASE['Indoor'], keep=False)
    assert none is None
    for i, o in enumerate(outs):
        want = torch.from_numpy(ge[f'{tag}_out{i}'])
        assert o.shape == want.shape and md(o, want) < 1e-4, (i, md(o, want))
    kept, _ = SE.net_fwd(P, x, num_res, training=False, tlsc=SE.TLSC_BASE['Indoor'], keep=True)
    assert all(torch.equal(a, b) for a, b in zip(kept, outs))                        # the box-mean operators stay on their per-op launches
    assert all(torch.equal(P[k].cpu(), sd[k]) for k in sd if SO.is_buffer(k))
