"""kernels.dihedral_gather / dihedral_mean (csrc/tdr_dihedral.hip) against their definition in inference.py (dihedral / dihedral_inverse and
the sequential fp32 sum), bit for bit.  Shapes: 5 x 7 and 1 x 9 (scalar paths, less than one LDS tile), 33 x 65 (crosses the 32 x 32 LDS
tile with remainders in both dimensions), 64 x 96 (the aligned float4 / word paths, several tiles)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(2, 3, 5, 7), (1, 1, 1, 9), (1, 6, 33, 65), (1, 3, 64, 96)]
GATHER_MASKS = [(0, 1, 2, 3), (4, 5, 6, 7)] + [(op,) for op in range(8)] + [(1, 2)]
MEAN_MASKS = [tuple(range(8)), (0, 1, 2, 3), (4, 5, 6, 7), (0, 5), (0, 3, 6)] + [(op,) for op in range(8)]


def _randn(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def _gathered(x, sel):
    from textualdegremoval_amd.inference import dihedral
    return torch.cat([dihedral(x, op).contiguous() for op in sel])


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_gather_float(shape):
    from textualdegremoval_amd import kernels as K
    x = _randn(*shape, seed=sum(shape))
    for sel in GATHER_MASKS:
        got = K.dihedral_gather(x, sel)
        want = _gathered(x, sel)
        assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want), sel


@pytest.mark.parametrize('shape', [(1, 3, 64, 96), (2, 3, 5, 7)], ids=lambda s: 'x'.join(map(str, s)))
def test_gather_float_from_a_source_one_float_past_a_16_byte_boundary(shape):
    from textualdegremoval_amd import kernels as K
    n = int(np.prod(shape))
    flat = _randn(n + 8, seed=7)
    assert flat.data_ptr() % 16 == 0
    x = flat[1:1 + n].view(shape)
    assert x.is_contiguous() and x.data_ptr() % 16 == 4
    for sel in GATHER_MASKS:
        assert torch.equal(K.dihedral_gather(x, sel), _gathered(x, sel)), sel


@pytest.mark.parametrize('swap', [True, False])
@pytest.mark.parametrize('C', [1, 3, 6])
@pytest.mark.parametrize('nhw', [(2, 5, 7), (1, 33, 65), (1, 64, 96)], ids=lambda s: 'x'.join(map(str, s)))
def test_gather_bytes(nhw, C, swap):
    from textualdegremoval_amd import kernels as K
    N, H, W = nhw
    u8 = torch.from_numpy(np.random.default_rng(H + C).integers(0, 256, size=(N, H, W, C), dtype=np.uint8)).cuda()
    planes = K.img_u8_to_planes(u8, swap_rb=swap)
    for sel in GATHER_MASKS:
        got = K.dihedral_gather(u8, sel, swap_rb=swap)
        assert torch.equal(got, _gathered(planes, sel)), sel


def test_gather_refuses_a_mixed_and_an_empty_mask():
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd._lib import TdrError
    x = _randn(1, 1, 4, 4, seed=1)
    with pytest.raises(TdrError, match='mixes'):
        K.dihedral_gather(x, (0, 4))
    with pytest.raises(TdrError, match='no op'):
        K.dihedral_gather(x, ())


def _members(shape, sel, seed, spread=None):
    """-> (straight [ks * N, C, H, W] or None, transposed [kt * N, C, W, H] or None, {op: its member [N, C, Ho, Wo]})"""
    N, C, H, W = shape
    members, stacks = {}, []
    for cls, hw in ((tuple(k for k in sel if k < 4), (H, W)), (tuple(k for k in sel if k >= 4), (W, H))):
        if not cls:
            stacks.append(None)
            continue
        gen = torch.Generator().manual_seed(seed + len(cls))
        if spread is None:
            t = torch.randn(len(cls) * N, C, *hw, generator=gen) * 0.37
        else:
            t = torch.rand(len(cls) * N, C, *hw, generator=gen) * (spread[1] - spread[0]) + spread[0]
        t = t.cuda()
        stacks.append(t)
        for i, op in enumerate(cls):
            members[op] = t[i * N:(i + 1) * N]
    return stacks[0], stacks[1], members


def _mean(members, sel):
    """the formula of the definition: s = inv(o_k0); s = s + inv(o_k1); ...; s / float32(n) -- a true division by a device tensor"""
    from textualdegremoval_amd.inference import dihedral_inverse
    s = None
    for op in sel:
        v = dihedral_inverse(members[op], op).contiguous()
        s = v if s is None else s + v
    return s / torch.tensor(float(len(sel)), dtype=torch.float32, device=s.device)


@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 3, 33, 65), (1, 3, 64, 96)], ids=lambda s: 'x'.join(map(str, s)))
def test_mean_float(shape):
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.inference import dihedral_inverse
    inexact = 0
    for sel in MEAN_MASKS:
        straight, transposed, members = _members(shape, sel, seed=len(sel))
        got = K.dihedral_mean(straight, transposed, sel, shape[0])
        want = _mean(members, sel)
        assert got.shape == tuple(shape) and torch.equal(got, want), sel
        if len(sel) == 1:
            assert torch.equal(got, dihedral_inverse(members[sel[0]], sel[0]))
        if len(sel) == 8:                                    # the sums round: another order of the additions gives other bits
            other = None
            for op in reversed(sel):
                v = dihedral_inverse(members[op], op)
                other = v if other is None else other + v
            inexact = int((other / 8 != want).sum())
    assert inexact > 0


@pytest.mark.parametrize('swap', [True, False])
@pytest.mark.parametrize('shape', [(2, 3, 5, 7), (1, 3, 33, 65), (1, 6, 64, 96), (1, 1, 8, 12)], ids=lambda s: 'x'.join(map(str, s)))
def test_mean_bytes(shape, swap):
    from textualdegremoval_amd import kernels as K
    for sel in MEAN_MASKS:
        straight, transposed, members = _members(shape, sel, seed=10 + len(sel), spread=(-0.2, 1.2))
        got = K.dihedral_mean(straight, transposed, sel, shape[0], u8=True, swap_rb=swap)
        f = K.dihedral_mean(straight, transposed, sel, shape[0])
        if len(sel) == 1:
            assert (f < 0).any() and (f > 1).any()           # both clamps are exercised
        assert got.dtype == torch.uint8 and torch.equal(got, K.planes_to_img_u8(f, swap_rb=swap)), sel


def test_mean_bytes_on_ties():
    """members that are multiples of 1 / 510: the mean of two of them times 255 is a multiple of 1 / 4 wherever the arithmetic is exact --
    many land on .5, which rounds to even only if the byte path rounds the very float the float path holds"""
    from textualdegremoval_amd import kernels as K
    N, C, H, W = 1, 3, 33, 65
    gen = torch.Generator().manual_seed(3)
    sel = (0, 5)
    a = (torch.randint(0, 511, (N, C, H, W), generator=gen).float() / 510.0).cuda()
    b = (torch.randint(0, 511, (N, C, W, H), generator=gen).float() / 510.0).cuda()
    f = K.dihedral_mean(a, b, sel, N)
    assert torch.equal(f, _mean({0: a, 5: b}, sel))
    prod = f * 255.0                                         # the float32 product the byte path rounds
    assert int((prod - prod.floor() == 0.5).sum()) > 100     # exact ties are there
    for swap in (True, False):
        assert torch.equal(K.dihedral_mean(a, b, sel, N, u8=True, swap_rb=swap), K.planes_to_img_u8(f, swap_rb=swap))
    one = ((torch.arange(3 * 16 * 32) % 511).float() / 510.0).view(1, 3, 16, 32).cuda()
    assert torch.equal(K.dihedral_mean(one, None, (0,), 1, u8=True), K.planes_to_img_u8(one))     # odd multiples of 1 / 510: u + .5 each
