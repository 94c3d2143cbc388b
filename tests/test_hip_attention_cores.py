"""Every instantiation of the channel-attention core kernels (csrc/tdr_mdta.hip) against the float64 reference of tests/_attn_core_ref.py:
kernels.mdta_softmax / mdta_bwd / tksa_softmax / tksa_bwd called directly on plain tensors -- no convolution launch, so the arithmetic mode
does not matter.  The kernels are built as <2> (head width c <= 128) and <3> (c <= 192); a lane owns the columns lane + 64 u, and the u = 1
slot carries data only when c > 64, the u = 2 slot only when c > 128.  The cases (tests/_attn_core_ref.SHAPES):
    (C, heads, HW, N) = (16, 2, 96, 2)    c = 8:   <2>, first slot only
                        (80, 1, 64, 2)    c = 80:  <2>, second slot, Cp = 96 != C
                        (160, 2, 64, 2)   c = 80:  <2>, second slot, two heads, backward LDS tile ~26 KB
                        (352, 2, 64, 2)   c = 176: <3>, third slot, two heads, backward LDS tile ~131 KB (above the 64 KB default limit)
                        (176, 1, 64, 3)   c = 176: <3>, Cp = 192 != C, N = 3
Bars: forward A 2e-6 absolute (the bar test_mdta_core_vs_torch holds MDTA to), times max(1, sum |am|) for TKSA.  W, dtemp, dam: 8 x the
deviation of the same reference evaluated in float32 on the CPU from the float64 one, relative to the tensor's maximum, never looser than
1e-4 of it.  Measured errors and bars are printed and persisted as attention_cores.json beside the other tests' margins (test_hip_full_size._record_margin).
TKSA rows whose float64 logits are within 2e-6 of each other at a top-k cut are left out (the fp32 kernel may select the other entry, a
discrete difference); at most 1 % of a case's rows.  Such a row must still sum to sum(am).  In the backward it takes with it its own row
and column of W, the k-side diagonal of its head and image (a column sum over the head's rows), its head's dtemp and the case's dam."""
import pytest
import torch

import _attn_core_ref as AR
from test_hip_full_size import _record_margin

pytestmark = pytest.mark.gpu
IDS = ['C%d-h%d-HW%d-N%d' % s for s in AR.SHAPES]
FWD_BAR = 2e-6

_cases = {}
_margins = {}


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels
    return kernels


def case(shape, kind, dead=None):
    """inputs and the float64 reference of one case, computed once and shared by the tests of that case (never modified)"""
    key = (shape, kind, dead)
    if key not in _cases:
        C, heads, HW, N = shape
        inp = AR.make_inputs(C, heads, HW, N, AR.SEEDS[shape], dead=dead)
        _cases[key] = (inp, AR.reference(inp, kind))
    return _cases[key]


def record(name, line):
    """print, and persist every measured margin of this module (the whole file is rewritten from what has run so far)"""
    print(line)
    _margins[name] = line
    _record_margin('attention_cores', [_margins[k] for k in sorted(_margins)])


def forward(K, inp, kind):
    G, ss, temp = inp['G'].cuda(), inp['ss'].cuda(), inp['temp'].cuda()
    if kind == 'mdta':
        return K.mdta_softmax(G, ss, temp, inp['heads'])
    return K.tksa_softmax(G, ss, temp, inp['am'].cuda(), inp['heads'])


def backward(K, inp, kind):
    G, ss, temp, dA = inp['G'].cuda(), inp['ss'].cuda(), inp['temp'].cuda(), inp['dA'].cuda()
    if kind == 'mdta':
        A, _ = K.mdta_softmax(G, ss, temp, inp['heads'])
        W, dtemp = K.mdta_bwd(G, ss, temp, A, dA, inp['heads'])
        return W, dtemp, None
    return K.tksa_bwd(G, ss, temp, inp['am'].cuda(), dA, inp['heads'])


def test_topk_sizes(K):
    for c in (8, 80, 176):
        assert list(K.tksa_ks(c)) == AR.tksa_ks(c) == [int(c / 2), int(c * 2 / 3), int(c * 3 / 4), int(c * 4 / 5)]


@pytest.mark.parametrize('kind', ['mdta', 'tksa'])
@pytest.mark.parametrize('shape', AR.SHAPES, ids=IDS)
def test_forward_vs_float64(K, shape, kind):
    C, heads, HW, N = shape
    c = C // heads
    inp, ref = case(shape, kind)
    A, AT = forward(K, inp, kind)
    Cp = AR.pad32(C)
    assert A.shape == AT.shape == (N, Cp, Cp)
    assert torch.equal(AT, A.transpose(1, 2))
    A = A.cpu()
    assert torch.isfinite(A).all()
    assert (A[:, ~AR.structure_A(C, heads)] == 0).all()                     # padding and off-head blocks: exactly zero
    bad = ref['bad']                                                         # [N, heads, c]
    assert int(bad.sum()) <= AR.TIE_CAP * bad.numel()
    scale = max(1.0, inp['am'].abs().sum().item()) if kind == 'tksa' else 1.0
    err = (AR.blocks(A[:, :C, :C], heads).double() - AR.blocks(ref['A'][:, :C, :C], heads)).abs().amax(dim=-1)     # per row
    kept = err[~bad].max().item()
    record(f'fwd {kind} {shape}', f'{kind} forward (C, heads, HW, N) = {shape}: max |A - ref| {kept:.3e}, bar {FWD_BAR * scale:.3e}; '
                                  f'{int(bad.sum())} of {bad.numel()} rows left out')
    assert kept <= FWD_BAR * scale
    if bad.any():
        rows = AR.blocks(A[:, :C, :C], heads).double().sum(dim=-1)[bad]
        assert (rows - inp['am'].double().sum()).abs().max().item() <= FWD_BAR * scale


@pytest.mark.parametrize('kind', ['mdta', 'tksa'])
@pytest.mark.parametrize('shape', AR.SHAPES, ids=IDS)
def test_backward_vs_float64(K, shape, kind):
    C, heads, HW, N = shape
    c = C // heads
    inp, ref = case(shape, kind)
    W, dtemp, dam = backward(K, inp, kind)
    Wp = AR.pad32(2 * C)
    assert W.shape == (N, Wp, Wp) and dtemp.shape == (heads, 1, 1)
    W, dtemp = W.cpu(), dtemp.cpu()
    assert torch.isfinite(W).all() and torch.isfinite(dtemp).all()
    assert (W[:, ~AR.structure_W(C, heads)] == 0).all()                     # everything outside the head blocks and the diagonal: exactly zero
    bad = ref['bad']
    assert int(bad.sum()) <= AR.TIE_CAP * bad.numel()
    keep = AR.structure_W(C, heads).expand(N, Wp, Wp).clone()
    for n, h, i in bad.nonzero().tolist():
        gi = h * c + i
        keep[n, gi, :] = False
        keep[n, :, gi] = False
        j = torch.arange(C + h * c, C + (h + 1) * c)
        keep[n, j, j] = False
    bars = AR.backward_bars(inp, kind, ref, keep)
    eW = AR.rel_dev(W, ref['W'], keep)
    line = f'{kind} backward (C, heads, HW, N) = {shape}: W {eW:.3e} (float32 reference {bars["W"][0]:.3e}, bar {bars["W"][1]:.3e})'
    ok_heads = ~bad.any(dim=2).any(dim=0)                                    # heads without a left-out row in any image
    eT = None
    if ok_heads.any():
        eT = ((dtemp.double() - ref['dtemp'])[ok_heads].abs().max() / ref['dtemp'].abs().max()).item()
        line += f'; dtemp {eT:.3e} ({bars["dtemp"][0]:.3e}, {bars["dtemp"][1]:.3e})'
    eA = None
    if kind == 'tksa':
        dam = dam.cpu()
        assert dam.shape == (4,) and torch.isfinite(dam).all()
        if not bad.any():
            eA = AR.rel_dev(dam, ref['dam'])
            line += f'; dam {eA:.3e} ({bars["dam"][0]:.3e}, {bars["dam"][1]:.3e})'
    record(f'bwd {kind} {shape}', line + f'; {int(bad.sum())} of {bad.numel()} rows left out')
    assert eW <= bars['W'][1]
    assert eT is None or eT <= bars['dtemp'][1]
    assert eA is None or eA <= bars['dam'][1]


def test_mdta_dead_channel(K):
    """one q row (in the second column slot) and one k row are zero in every image: G row / column 0 and ss 0.  The A row is uniform 1/c,
    W[i, i] = 0 for the two channels, everything is finite.  The clamped norm 1e-12 puts the dead row and column of W at 1e12 times the
    rest (1e24 where they cross), so W is compared as D W D, D = 1e-12 / sqrt(HW) at the two dead channels and 1 elsewhere: W carries 1 / norm, and a live channel's
    norm is about sqrt(HW), so this puts every entry at the live scale and the maximum and the float32 deviation are taken over the whole tensor."""
    shape = (80, 1, 64, 2)
    C, heads, HW, N = shape
    iq, jk = 70, 3
    inp, ref = case(shape, 'mdta', dead=(0, iq, jk))
    assert (inp['ss'][:, iq] == 0).all() and (inp['ss'][:, C + jk] == 0).all() and (inp['G'][:, iq, :] == 0).all() and (inp['G'][:, :, jk] == 0).all()
    A, AT = forward(K, inp, 'mdta')
    assert torch.equal(AT, A.transpose(1, 2))
    A = A.cpu()
    assert torch.isfinite(A).all()
    assert (A[:, iq, :C].double() - 1.0 / C).abs().max().item() <= FWD_BAR
    assert (A.double() - ref['A']).abs().max().item() <= FWD_BAR
    W, dtemp, _ = backward(K, inp, 'mdta')
    W, dtemp = W.cpu(), dtemp.cpu()
    Wp = W.shape[-1]
    assert torch.isfinite(W).all() and torch.isfinite(dtemp).all()
    assert (W[:, iq, iq] == 0).all() and (W[:, C + jk, C + jk] == 0).all()
    S = AR.structure_W(C, heads)
    assert (W[:, ~S] == 0).all()
    d = torch.ones(Wp, dtype=torch.float64)
    d[iq] = d[C + jk] = AR.NORM_EPS / HW ** 0.5
    scale = d[:, None] * d[None, :]
    bars = AR.backward_bars(inp, 'mdta', ref, scale_W=scale)
    eW = AR.rel_dev(W, ref['W'], scale=scale)
    eT = AR.rel_dev(dtemp, ref['dtemp'])
    record('dead mdta', f'mdta dead channel (C, heads, HW, N) = {shape}: W (dead row and column times 1e-12 / sqrt(HW)) {eW:.3e} (float32 reference '
                        f'{bars["W"][0]:.3e}, bar {bars["W"][1]:.3e}); dtemp {eT:.3e} (float32 reference {bars["dtemp"][0]:.3e}, bar 1.000e-04)')
    assert eW <= bars['W'][1]
    # dtemp here is one number, so the float32 deviation is a sample of one (7.7e-8 on one host, 4.6e-7 on another, the kernel 7.5e-7): it
    # is printed, and the case holds dtemp to the project's 1e-4 (test_mdta_core_vs_torch); the five regular cases hold it to the 8 x bar
    assert eT <= 1e-4
