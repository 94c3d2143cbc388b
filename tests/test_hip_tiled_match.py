"""Matched tiled inference on the GPU: `run_tiled(..., matcher=m)` restores every tile against the window of its image's ref that
`m.match(tile, ref[n])` picks.  The contract is bit-identity with match() per tile -- (ref_in, index, corr) -- and, end to end, a
composite built here from the CPU oracle's windows (oracle.dino_oracle.match_reference_window) under the blend bound of
tests/test_hip_tiled_inference.py.

The small matcher of tests/test_hip_dino.py (embed 32, depth 2, 2 heads) and the width-8 guided network that takes tiles of 128."""
import os

import numpy as np
import pytest
import torch

import test_hip_infer_session as TS
from oracle import dino_oracle as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound of tests/test_hip_tile_kernels.py: at most 9 terms of two roundings each, 8 additions, weights summing to ~1
BLEND_ULPS = 16 * 2.0 ** -24
SD = D.synth_vit_params(32, 2, 2, seed=11)
_matchers = {}


@pytest.fixture(autouse=True)
def bx3():
    from textualdegremoval_amd import kernels as K
    prev = K.MATH
    K.set_math('bx3')
    yield
    K.set_math(prev)


def _matcher(math='bx3'):
    """the frozen weights are packed for kernels.MATH at construction: built (once) under the arithmetic it will run in"""
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.dino import DinoMatcher
    K.set_math(math)
    if math not in _matchers:
        _matchers[math] = DinoMatcher(SD, torch.device('cuda'), heads=2, linear_math=math)
    return _matchers[math]


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


# ---------------------------------------------------------------------------------------------------------------- kernels
@pytest.mark.parametrize('Wr', [96, 128])
def test_window_resize_is_resize_of_unfold(Wr):
    from textualdegremoval_amd import kernels as K
    ref = _rand(2, 3, 96, Wr, seed=1)
    win, N = K.unfold_windows(ref, 48, 12)
    assert N == 5 * ((Wr - 48) // 12 + 1)
    want = K.resize_bilinear(win, 56, 56).view(2, N, 3, 56, 56)
    for n0, count in ((0, N), (7, 5), (N - 1, 1)):
        got = K.window_resize(ref, 48, 12, n0, count, 56, 56)
        assert got.shape == (2 * count, 3, 56, 56)
        assert torch.equal(got.view(2, count, 3, 56, 56), want[:, n0:n0 + count]), (n0, count)
    from textualdegremoval_amd._lib import TdrError
    with pytest.raises(TdrError):
        K.window_resize(ref, 48, 12, N - 1, 2, 56, 56)                       # one window past the grid: refused, nothing launched


def test_bank_does_not_depend_on_the_chunk():
    m = _matcher()
    ref = _rand(2, 3, 96, 128, seed=2)
    a, b = m.window_bank(ref, 48, chunk=4), m.window_bank(ref, 48, chunk=64)
    assert (a.ny, a.nx, a.stride, a.t, a.T) == (5, 7, 12, 48, 16) == (b.ny, b.nx, b.stride, b.t, b.T)
    assert a.feats.shape == (2 * 35, 32, 1, 32) and torch.equal(a.feats, b.feats)


@pytest.mark.parametrize('math', ['bx3', 'f32'])
def test_match_bank_is_match_per_slot(math):
    m = _matcher(math)
    ref = _rand(2, 3, 96, 128, seed=3)
    tiles = _rand(4, 3, 48, 48, seed=4)
    tiles = torch.cat([tiles, tiles[3:4]])                                   # the padding slot of a last batch repeats a tile
    rows = torch.tensor([0, 0, 1, 1, 1], dtype=torch.int32, device='cuda')
    ref_in, index, corr = m.match_bank(tiles, m.window_bank(ref, 48), rows, ref)
    assert ref_in.shape == (5, 3, 48, 48) and index.dtype == torch.int32 and corr.shape == (5, 35)
    for b, r in enumerate(rows.tolist()):
        w_ref_in, w_index, w_corr = m.match(tiles[b:b + 1], ref[r:r + 1])
        assert torch.equal(corr[b:b + 1], w_corr), (b, (corr[b:b + 1] - w_corr).abs().max().item())
        assert torch.equal(index[b:b + 1], w_index) and torch.equal(ref_in[b:b + 1], w_ref_in), b
    assert torch.equal(corr[4], corr[3]) and torch.equal(ref_in[4], ref_in[3])


def test_ties_go_to_the_first_window():
    m = _matcher()
    ref = _rand(1, 3, 96, 12, seed=5).repeat(1, 1, 1, 9)                     # columns of period 12 = the stride: a row of equal windows
    assert ref.shape == (1, 3, 96, 108)
    tiles = _rand(2, 3, 48, 48, seed=6)
    rows = torch.zeros(2, dtype=torch.int32, device='cuda')
    bank = m.window_bank(ref, 48)
    assert (bank.ny, bank.nx) == (5, 6)
    ref_in, index, corr = m.match_bank(tiles, bank, rows, ref)
    c = corr.view(2, 5, 6)
    assert torch.equal(c, c[:, :, :1].expand(2, 5, 6))                       # the ties are exact
    assert all(int(i) % 6 == 0 for i in index.tolist())
    for b in range(2):
        w_ref_in, w_index, _ = m.match(tiles[b:b + 1], ref)
        assert torch.equal(index[b:b + 1], w_index) and torch.equal(ref_in[b:b + 1], w_ref_in)


def test_bank_kernel_on_long_bands_and_many_slots():
    """tdr_token_match_bank against tdr_token_match on synthetic token maps that the small matcher does not reach: bands of 5 rows x
    1056 columns (two staging rounds, the second partly filled), nine slots of one image (two passes over its slices), an image
    without a slot, and a slot whose row names no image (corr 0, index -1, zeros)"""
    from textualdegremoval_amd import kernels as K
    g = torch.Generator().manual_seed(7)
    Dm, T1, LD, Nw = 200, 1030, 1056, 3
    ref = _rand(3, 3, 32, 48, seed=8)                                        # windows of 32 at stride 8: a grid of 1 x 3
    win, N = K.unfold_windows(ref, 32, 8)
    assert N == Nw
    bank = torch.randn(3 * Nw, Dm, LD // 32, 32, generator=g).cuda()
    fl = torch.randn(11, Dm, LD // 32, 32, generator=g).cuda()
    rows = torch.tensor([2] + [0] * 9 + [5], dtype=torch.int32, device='cuda')
    corr, index, ref_in = K.token_match_bank(fl, bank, rows, ref, 32, 8, 3, T1)
    for b, r in enumerate(rows.tolist()[:10]):
        w_corr, w_index, w_ref_in = K.token_match(fl[b:b + 1], bank[r * Nw:(r + 1) * Nw], win[r * Nw:(r + 1) * Nw], Nw, T1)
        assert torch.equal(corr[b:b + 1], w_corr) and torch.equal(index[b:b + 1], w_index) and torch.equal(ref_in[b:b + 1], w_ref_in), b
    assert int(index[10]) == -1 and not ref_in[10].any() and not corr[10].any()


# ---------------------------------------------------------------------------------------------------------------- sessions
def _planted():
    g = torch.Generator().manual_seed(70)
    ref = torch.rand(1, 3, 192, 256, generator=g)
    lq = (ref[:, :, 32:192, 32:224] + 0.02 * torch.randn(1, 3, 160, 192, generator=g)).clamp(0, 1)
    return lq, ref


@pytest.fixture(scope='module')
def planted():
    """the oracle's choice per tile, computed once on the CPU: (lq, ref, [(y0, x0, ref_in, index, corr)])"""
    lq, ref = _planted()
    per_tile = []
    for y0 in (0, 32):
        for x0 in (0, 64):
            ref_in, idx, corr = D.match_reference_window(SD, lq[:, :, y0:y0 + 128, x0:x0 + 128].contiguous(), ref, heads=2)
            per_tile.append((y0, x0, ref_in, int(idx), corr))
    return lq, ref, per_tile


def matched_composite(net, lq, ref_ins, tile, overlap, tile_batch):
    """`composite` of tests/test_hip_tiled_inference.py for one image, with the tile's own ref_in (ref_ins[i], a CPU tensor
    [1,3,t,t]) in place of the ref row: the same padded batches, each through a session of its own, blended in float64"""
    from textualdegremoval_amd.inference import InferenceSession, full_size, tile_batches, tile_starts, tile_weights
    _, _, H, W = lq.shape
    (ys, th), (xs, tw) = tile_starts(H, tile, overlap), tile_starts(W, tile, overlap)
    x = lq.cpu().numpy()
    where = [(y0, x0) for y0 in ys for x0 in xs]
    assert len(where) == len(ref_ins)
    sess = InferenceSession(net, max_graphs=0)
    outs = {}
    for batch in tile_batches(len(where), tile_batch):
        tiles = np.stack([x[0, :, y0:y0 + th, x0:x0 + tw] for y0, x0 in (where[i] for i in batch)])
        refs = torch.cat([ref_ins[i] for i in batch]).cuda()
        out = full_size(sess(torch.from_numpy(tiles).cuda(), refs)).cpu().numpy()
        for slot, i in enumerate(batch):
            outs.setdefault(i, out[slot])                                    # (a padding slot repeats a tile: the first one counts)
    sess.release()
    (fy, cy, wy), (fx, cx, wx) = tile_weights(H, tile, overlap), tile_weights(W, tile, overlap)
    want = np.zeros((1, outs[0].shape[0], H, W), np.float64)
    for i, (y0, x0) in enumerate(where):
        yy, xx = np.arange(y0, y0 + th), np.arange(x0, x0 + tw)
        iy, ix = ys.index(y0), xs.index(x0)
        w = wy[yy, iy - fy[yy]].astype(np.float64)[:, None] * wx[xx, ix - fx[xx]].astype(np.float64)[None, :]
        want[0, :, y0:y0 + th, x0:x0 + tw] += w * outs[i].astype(np.float64)
    once = (cy == 1)[:, None] & (cx == 1)[None, :]
    return want, once, max(np.abs(o).max() for o in outs.values())


def agrees(got, want, once, top):
    got = got.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want).max()
    print(f'max |run_tiled - composite| {err:.3e}, bound {BLEND_ULPS * top:.3e} (max |tile output| {top:.3f}); '
          f'{once.mean():.2f} of the pixels covered once')
    assert got.shape == want.shape and err <= BLEND_ULPS * top
    assert np.array_equal(got[:, :, once].view(np.uint32), want.astype(np.float32)[:, :, once].view(np.uint32))


def test_planted_matches_end_to_end(planted):
    from textualdegremoval_amd.inference import InferenceSession
    m = _matcher()
    net, _, _ = TS._guided('net_w8_128_wrap', None)
    lq, ref, per_tile = planted
    assert [(y0, x0) for y0, x0, *_ in per_tile] == [(0, 0), (0, 64), (32, 0), (32, 64)]
    margins = [float(torch.topk(c[0], 2).values.diff().abs()) for *_, c in per_tile]
    print('oracle windows', [i for *_, i, _ in per_tile], 'top-1 / top-2 margins', [f'{v:.4f}' for v in margins])
    assert [i for *_, i, _ in per_tile] == [6, 8, 11, 13]
    lq_d, ref_d = lq.cuda(), ref.cuda()
    # the matcher alone, per tile, against the oracle
    tiles = torch.cat([lq_d[:, :, y0:y0 + 128, x0:x0 + 128] for y0, x0, *_ in per_tile]).contiguous()
    ref_in, index, corr = m.match_bank(tiles, m.window_bank(ref_d, 128), torch.zeros(4, dtype=torch.int32, device='cuda'), ref_d)
    for b, (_, _, o_ref_in, o_idx, o_corr) in enumerate(per_tile):
        assert int(index[b]) == o_idx and torch.equal(ref_in[b:b + 1].cpu(), o_ref_in)
        assert (corr[b:b + 1].cpu() - o_corr).abs().max().item() < 1e-5
    # the session: one batch of four, three calls -- eager, capture + replay, replay
    sess = InferenceSession(net)
    outs = [sess.run_tiled(lq_d, ref_d, tile=128, overlap=32, tile_batch=4, matcher=m) for _ in range(3)]
    assert sess.captures == 1 and sess.replays == 2 and len(sess.graphs) == 1
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    lm = sess.last_match
    assert lm['index'].dtype == torch.int32 and lm['index'].tolist() == [6, 8, 11, 13] and lm['grid'] == (3, 5, 32)
    assert lm['corr'].shape == (4, 15) and torch.equal(lm['corr'], corr) and lm['corr'].is_cuda
    want, once, top = matched_composite(net, lq, [p[2] for p in per_tile], 128, 32, 4)
    assert once.any() and not once.all()
    agrees(outs[0], want, once, top)
    # two batches of three, padding slots dropped from the record
    got3 = sess.run_tiled(lq_d, ref_d, tile=128, overlap=32, tile_batch=3, matcher=m)
    assert sess.last_match['index'].tolist() == [6, 8, 11, 13] and torch.equal(sess.last_match['corr'], corr)
    agrees(got3, *matched_composite(net, lq, [p[2] for p in per_tile], 128, 32, 3))
    # packed weights only
    zero = InferenceSession(net, max_graphs=0)
    assert torch.equal(zero.run_tiled(lq_d, ref_d, tile=128, overlap=32, tile_batch=4, matcher=m), outs[0]) and zero.captures == 0
    for s in (sess, zero):
        s.release()


def test_non_square_ref_runs_matched_only():
    from textualdegremoval_amd.inference import InferenceSession
    m = _matcher()
    net, _, _ = TS._guided('net_w8_128_wrap', None)
    lq, ref = _rand(1, 3, 128, 128, seed=71), _rand(1, 3, 128, 384, seed=72)
    sess = InferenceSession(net)
    out = sess.run_tiled(lq, ref, tile=128, tile_batch=1, matcher=m)
    lm = sess.last_match
    assert out.shape == lq.shape and lm['grid'] == (1, 9, 32) and lm['corr'].shape == (1, 9)
    w = int(lm['index'][0])
    assert 0 <= w < 9
    assert torch.equal(out, sess(lq, ref[:, :, :, 32 * w:32 * w + 128].contiguous()))      # one tile, one image: the plain call on that window
    with pytest.raises(ValueError, match='MASA geometry must be square'):
        sess.run_tiled(lq, ref, tile=128, tile_batch=1)
    sess.release()


def test_one_graph_for_every_image_and_ref_size():
    from textualdegremoval_amd.inference import InferenceSession
    m = _matcher()
    net, _, _ = TS._guided('net_w8_128_wrap', None)
    sess = InferenceSession(net)
    a = sess.run_tiled(_rand(1, 3, 160, 192, seed=73), _rand(1, 3, 192, 256, seed=74), tile=128, overlap=32, tile_batch=2, matcher=m)
    assert sess.last_match['grid'] == (3, 5, 32) and sess.last_match['index'].shape == (4,)
    b = sess.run_tiled(_rand(1, 3, 128, 200, seed=75), _rand(1, 3, 128, 384, seed=76), tile=128, overlap=32, tile_batch=2, matcher=m)
    assert sess.last_match['grid'] == (1, 9, 32) and sess.last_match['index'].shape == (2,)
    assert a.shape == (1, 3, 160, 192) and b.shape == (1, 3, 128, 200)
    assert sess.captures == 1 and len(sess.graphs) == 1 and sess.replays == 2
    sess.release()


def test_a_ref_of_one_window_skips_the_matcher(monkeypatch):
    from textualdegremoval_amd.inference import InferenceSession
    m = _matcher()
    net, _, _ = TS._guided('net_w8_128_wrap', None)
    lq, ref = _rand(1, 3, 160, 192, seed=77), _rand(1, 3, 128, 128, seed=78)
    calls, orig = [], m.tokens
    monkeypatch.setattr(m, 'tokens', lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    sess = InferenceSession(net)
    want = sess.run_tiled(lq, ref, tile=128, overlap=32, tile_batch=4)
    got = sess.run_tiled(lq, ref, tile=128, overlap=32, tile_batch=4, matcher=m)
    assert torch.equal(got, want) and not calls
    assert sess.last_match['index'].tolist() == [0, 0, 0, 0] and sess.last_match['grid'] == (1, 1, 32)
    sess.release()


def test_matcher_arguments_are_validated():
    from textualdegremoval_amd.inference import InferenceSession
    m = _matcher()
    net, _, _ = TS._guided('net_w8_128_wrap', None)
    sess = InferenceSession(net)
    lq = _rand(1, 3, 160, 192, seed=79)
    with pytest.raises(TypeError):
        sess.run_tiled(lq, tile=128, matcher=m)                               # no ref
    with pytest.raises(TypeError):
        sess.run_tiled(lq, _rand(1, 3, 192, 256, seed=80).double(), tile=128, matcher=m)
    with pytest.raises(ValueError):
        sess.run_tiled(lq, _rand(1, 4, 192, 256, seed=80), tile=128, matcher=m)
    with pytest.raises(ValueError, match='100 x 256'):
        sess.run_tiled(lq, _rand(1, 3, 100, 256, seed=80), tile=128, matcher=m)          # a ref smaller than the tile
    with pytest.raises(NotImplementedError):
        sess.run_tiled(lq, _rand(1, 3, 192, 256, seed=80), tile=(128, 96), matcher=m)
    sess.release()


def test_run_tiled_u8_matched_converts_the_ref_once(monkeypatch):
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.inference import InferenceSession
    m = _matcher()
    net, _, _ = TS._guided('net_w8_128_wrap', None)
    rng = np.random.default_rng(81)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(1, 160, 192, 3), dtype=np.uint8)).cuda()
    ref = torch.from_numpy(rng.integers(0, 256, size=(1, 192, 256, 3), dtype=np.uint8)).cuda()
    sess = InferenceSession(net)
    want = K.planes_to_img_u8(sess.run_tiled(K.img_u8_to_planes(u8), K.img_u8_to_planes(ref), tile=128, overlap=32, tile_batch=2, matcher=m))
    index = sess.last_match['index'].clone()
    calls, orig = [], K.img_u8_to_planes
    monkeypatch.setattr(K, 'img_u8_to_planes', lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    got = sess.run_tiled_u8(u8, ref, tile=128, overlap=32, tile_batch=2, matcher=m)
    assert got.dtype == torch.uint8 and torch.equal(got, want) and len(calls) == 1
    assert torch.equal(sess.last_match['index'], index)
    sess.release()


def test_step_model_validates_matched_tiles(monkeypatch, tmp_path):
    """`val: {tile: 48, tile_match: true}` on the synthetic debug option file, the small matcher as net_ext: refs of 128 x 128 hold 49
    windows of 48; one nondist_validation reports the PSNR of run_tiled(..., matcher=net_ext), from a single graph"""
    import torch.nn.functional as F
    from textualdegremoval_amd.metrics import calculate_psnr, tensor2img
    from textualdegremoval_amd.models import create_model
    from textualdegremoval_amd.utils.utils_options import parse
    monkeypatch.setenv('TDR_EXPERIMENTS_ROOT', str(tmp_path))
    opt = parse(os.path.join(ROOT, 'tests', 'data', 'train_nafnet_ref_synthetic_debug.yml'), is_train=True)
    opt['dist'] = False
    opt['val'].update(tile=48, tile_overlap=16, tile_batch=2, tile_match=True)
    model = create_model(opt)
    assert model.net_ext is None
    data = []
    for i, (H, W) in enumerate(((100, 76), (64, 120))):
        data.append({'lq': _rand(1, 3, H, W, seed=40 + i), 'gt': _rand(1, 3, H, W, seed=50 + i), 'ref': _rand(1, 3, 128, 128, seed=60 + i)})
    with pytest.raises(ValueError, match='path.pretrain_dino'):
        model.nondist_validation(data, 1, None, False, True, True)
    model.net_ext = _matcher()
    psnr = model.nondist_validation(data, 1, None, False, True, True)
    sessions = list(model._val_sessions.values())
    assert len(sessions) == 1 and sessions[0].captures == 1 and len(sessions[0].graphs) == 1
    assert sessions[0].last_match['grid'] == (7, 7, 12) and sessions[0].last_match['corr'].shape[1] == 49
    by_hand = []
    for d in data:
        H, W = d['lq'].shape[2:]
        padded = F.pad(d['lq'], (0, -W % 8, 0, -H % 8), 'reflect')
        out = sessions[0].run_tiled(padded, d['ref'], tile=48, overlap=16, tile_batch=2, matcher=model.net_ext)[:, :, :H, :W]
        by_hand.append(calculate_psnr(tensor2img(out.cpu(), rgb2bgr=True), tensor2img(d['gt'].cpu(), rgb2bgr=True), crop_border=0,
                                      test_y_channel=False))
    assert torch.equal(model.output, out)
    assert psnr == model.metric_results['psnr'] == sum(by_hand) / 2
    assert sessions[0].captures == 1
