"""csrc/tdr_tile.hip alone, no network: kernels.tile_gather against numpy slicing (bit-exact; the byte source against the reference's
float32(u) / 255 and against slices of kernels.img_u8_to_planes) and kernels.tile_blend against the same sum in float64 from the same
float32 tables."""
import numpy as np
import pytest
import torch

from textualdegremoval_amd.inference import TilePlan

pytestmark = pytest.mark.gpu
# per element: at most 9 terms, each with one rounding of wy * wx and one of the product with v, 8 additions, sum of weights ~ 1 -- about
# 10 ulp of the largest tile value; 16 leaves room for contraction either way
BLEND_ULPS = 16 * 2.0 ** -24


def _plan(N, H, W, tile, overlap, tile_batch=4):
    return TilePlan(N, H, W, (tile, tile) if isinstance(tile, int) else tile, overlap, tile_batch, 'cuda')


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def np_gather(planes, plan):
    """planes [N,C,H,W] -> the tiles of plan.table by slicing"""
    return np.stack([planes[n, :, y0:y0 + plan.th, x0:x0 + plan.tw] for n, y0, x0 in plan.table.cpu().numpy()])


def np_blend64(tiles, N, H, W, plan):
    """the blend in float64 from the plan's float32 tables; also the map of pixels covered by one tile in both dimensions"""
    (ys, yi, yw), (xs, xi, xw) = [[t.cpu().numpy() for t in tabs] for tabs in (plan.ytabs, plan.xtabs)]
    out = np.zeros((N, tiles.shape[1], H, W), np.float64)
    for n in range(N):
        for iy, y0 in enumerate(ys):
            yy = np.arange(y0, y0 + plan.th)
            wy = yw[yy, iy - yi[yy, 0]].astype(np.float64)
            assert ((iy >= yi[yy, 0]) & (iy < yi[yy, 0] + yi[yy, 1])).all()
            for ix, x0 in enumerate(xs):
                xx = np.arange(x0, x0 + plan.tw)
                wx = xw[xx, ix - xi[xx, 0]].astype(np.float64)
                out[n, :, y0:y0 + plan.th, x0:x0 + plan.tw] += wy[:, None] * wx[None, :] * tiles[(n * plan.ny + iy) * plan.nx + ix].astype(np.float64)
    once = (yi[:, 1] == 1)[:, None] & (xi[:, 1] == 1)[None, :]
    return out, once


# ------------------------------------------------------------------ gather
@pytest.mark.parametrize('shape', [(2, 3, 37, 50, 16), (1, 1, 37, 50, 16), (1, 3, 36, 48, 16), (1, 3, 12, 50, 16), (1, 6, 21, 40, (8, 12))])
def test_gather_float_bit_exact(shape):
    from textualdegremoval_amd import kernels as K
    N, C, H, W, tile = shape
    plan = _plan(N, H, W, tile, 4)
    x = np.random.default_rng(1).standard_normal((N, C, H, W)).astype(np.float32)
    got = K.tile_gather(torch.from_numpy(x).cuda(), plan.table, plan.th, plan.tw).cpu().numpy()
    want = np_gather(x, plan)
    assert plan.table.shape[0] % 4 == 0 and got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    if (H, W) == (12, 50):
        assert (plan.th, plan.tw) == (12, 16)                                # a rectangular tile: the image is lower than the tile


@pytest.mark.parametrize('swap', [False, True])
@pytest.mark.parametrize('shape', [(2, 37, 50, 3), (1, 36, 48, 3), (1, 37, 50, 1), (1, 36, 48, 6), (1, 12, 50, 3)])
def test_gather_u8_bit_exact(shape, swap):
    """W = 50: byte by byte; 36 x 48 with starts 0, 12, 24, 32: the 32-bit word path"""
    from textualdegremoval_amd import kernels as K
    N, H, W, C = shape
    plan = _plan(N, H, W, 16, 4)
    if W == 48:
        assert (plan.table[:, 2] % 4 == 0).all()
    u8 = np.random.default_rng(2).integers(0, 256, size=shape, dtype=np.uint8)
    u8.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)                    # every byte value
    dev = torch.from_numpy(u8).cuda()
    got = K.tile_gather(dev, plan.table, plan.th, plan.tw, swap_rb=swap).cpu().numpy()
    planes = u8.astype(np.float32) / np.float32(255)
    if C == 3 and swap:
        planes = planes[..., ::-1]
    want = np_gather(planes.transpose(0, 3, 1, 2), plan)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    want_k = np_gather(K.img_u8_to_planes(dev, swap_rb=swap).cpu().numpy(), plan)
    assert np.array_equal(_bits(got), _bits(want_k))


def test_gather_refuses_a_tile_larger_than_the_image():
    from textualdegremoval_amd import kernels as K
    table = torch.zeros(1, 3, dtype=torch.int32, device='cuda')
    with pytest.raises(RuntimeError):
        K.tile_gather(torch.zeros(1, 3, 8, 8, device='cuda'), table, 16, 8)


# ------------------------------------------------------------------ blend
GRIDS = [(2, 3, 37, 50, 16, 4), (1, 3, 36, 48, 16, 4), (1, 3, 12, 50, 16, 4), (1, 3, 49, 33, 16, 8), (1, 2, 70, 130, 48, 16)]


@pytest.mark.parametrize('grid', GRIDS)
def test_blend_against_float64(grid):
    from textualdegremoval_amd import kernels as K
    N, C, H, W, tile, overlap = grid
    plan = _plan(N, H, W, tile, overlap)
    if (H, W, overlap) == (49, 33, 8):
        assert plan.ytabs[2].shape[1] == 3 and plan.xtabs[2].shape[1] == 3                # the 3 x 3 cover
    tiles = (np.random.default_rng(3).standard_normal((plan.n_tiles, C, plan.th, plan.tw)) * 3).astype(np.float32)
    got = K.tile_blend(torch.from_numpy(tiles).cuda(), N, H, W, plan.ytabs, plan.xtabs).cpu().numpy()
    want, once = np_blend64(tiles, N, H, W, plan)
    err = np.abs(got.astype(np.float64) - want).max()
    bound = BLEND_ULPS * np.abs(tiles).max()
    print(f'{grid}: max |blend - float64| {err:.3e}, bound {bound:.3e}; {once.mean():.2f} of the pixels covered once')
    assert got.shape == want.shape and err <= bound
    assert once.any() and np.array_equal(_bits(got[:, :, once]), _bits(want.astype(np.float32)[:, :, once]))     # covered once: a copy
    const = torch.full(tiles.shape, 0.7, dtype=torch.float32, device='cuda')
    flat = K.tile_blend(const, N, H, W, plan.ytabs, plan.xtabs).cpu().numpy()
    assert np.abs(flat.astype(np.float64) - np.float64(np.float32(0.7))).max() <= BLEND_ULPS * 0.7


@pytest.mark.parametrize('grid', [(2, 3, 48, 32, 16, 0), (1, 3, 37, 50, 16, 0), (1, 3, 12, 12, 16, 4), (1, 1, 9, 7, 16, 4)])
def test_blend_bit_exact_without_overlap_and_for_a_single_tile(grid):
    """overlap 0 (the clamped last tile of 37 / 50 still lies over its neighbour: both hold the image there) and one tile: copies"""
    from textualdegremoval_amd import kernels as K
    N, C, H, W, tile, overlap = grid
    plan = _plan(N, H, W, tile, overlap)
    x = (np.random.default_rng(4).standard_normal((N, C, H, W)) * 3).astype(np.float32)
    x[0, 0, 0, :4] = [0.0, -0.0, 1.0, -1.0]                                  # the sign of a zero survives
    tiles = np_gather(x, plan)[:plan.n_tiles]
    if (H, W) == (12, 12):
        assert plan.n_tiles == 1
    if overlap == 0 and H % tile == 0 and W % tile == 0:
        assert all((t[2] == 1.0).all().item() for t in (plan.ytabs, plan.xtabs))
    got = K.tile_blend(torch.from_numpy(tiles).cuda(), N, H, W, plan.ytabs, plan.xtabs).cpu().numpy()
    if overlap == 0 and (H % tile or W % tile):
        # weights 1/2 + 1/2 of equal values where the clamped tile overlaps: v/2 + v/2 = v exactly
        assert np.array_equal(got, x)
    else:
        assert np.array_equal(_bits(got), _bits(x))
