"""The tile plan of InferenceSession.run_tiled, no GPU: where the tiles start (inference.tile_starts), the per-pixel blend table
(tile_weights) and the batches of one size (tile_batches)."""
import numpy as np
import pytest

from textualdegremoval_amd.inference import tile_batches, tile_starts, tile_weights

CASES = [(37, 16, 4), (50, 16, 4), (12, 16, 4), (48, 16, 0), (49, 16, 8), (33, 16, 8), (70, 48, 16), (130, 48, 16)]


def test_tile_starts_vectors():
    assert tile_starts(37, 16, 4) == ([0, 12, 21], 16)
    assert tile_starts(50, 16, 4) == ([0, 12, 24, 34], 16)
    assert tile_starts(12, 16, 4) == ([0], 12)
    assert tile_starts(49, 16, 8) == ([0, 8, 16, 24, 32, 33], 16)


@pytest.mark.parametrize('bad', [(37, 16, -1), (37, 16, 16), (37, 0, 0)])
def test_tile_starts_refuses(bad):
    with pytest.raises(ValueError):
        tile_starts(*bad)


@pytest.mark.parametrize('case', CASES)
def test_tile_weights_table(case):
    L, tile, overlap = case
    starts, t = tile_starts(L, tile, overlap)
    first, cnt, w = tile_weights(L, tile, overlap)
    assert first.dtype == cnt.dtype == np.int32 and w.dtype == np.float32
    assert first.shape == cnt.shape == (L,) and w.shape == (L, cnt.max())
    assert all(0 <= s <= L - t for s in starts) and starts == sorted(set(starts))       # every tile inside, all of one length
    for y in range(L):
        covering = [i for i, s in enumerate(starts) if s <= y < s + t]
        assert covering, f'pixel {y} is not covered'
        assert covering == list(range(first[y], first[y] + cnt[y])), (y, covering)       # contiguous, and the table says so
        assert abs(w[y, :cnt[y]].astype(np.float64).sum() - 1.0) <= 2.0 ** -24 and (w[y, :cnt[y]] > 0).all()
        assert (w[y, cnt[y]:] == 0).all()
        r = [min(y - starts[i] + 1, t - (y - starts[i]), overlap + 1) for i in covering]                  # the rule, restated
        assert np.array_equal(w[y, :cnt[y]], (np.asarray(r, np.float64) / np.float64(sum(r))).astype(np.float32))
    assert (w[cnt == 1, 0] == np.float32(1.0)).all()
    if overlap == 0:
        assert (cnt == 1).all() and (w == np.float32(1.0)).all()
    if L > t and (L - t) % (t - overlap) == 0:                                           # the clamped tile is a regular one: y -> L - 1 - y
        n = len(starts)
        assert np.array_equal(cnt, cnt[::-1]) and np.array_equal(first + cnt - 1, n - 1 - first[::-1])
        for y in range(L):
            assert np.array_equal(w[y, :cnt[y]], w[L - 1 - y, :cnt[y]][::-1]), y


def test_cover_is_not_bounded_by_two():
    for case in ((49, 16, 8), (33, 16, 8), (41, 16, 8)):
        first, cnt, w = tile_weights(*case)
        assert cnt.max() == 3 and w.shape[1] == 3, case


def test_tile_batches():
    assert tile_batches(5, 4) == [[0, 1, 2, 3], [4, 4, 4, 4]]
    assert tile_batches(2, 4) == [[0, 1, 1, 1]]
    assert tile_batches(8, 4) == [[0, 1, 2, 3], [4, 5, 6, 7]]
    assert tile_batches(3, 1) == [[0], [1], [2]]
