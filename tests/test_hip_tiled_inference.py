"""InferenceSession.run_tiled / run_tiled_u8 on the GPU against a composite built here: the tiles sliced in numpy, formed into the same
padded batches, each batch through `sess(batch)`, blended in float64 with the host tables (inference.tile_starts / tile_weights /
tile_batches).  The composite uses the same batch composition -- a sample's bits are not assumed independent of its batch-mates.

The NAFNet-w32 cases run tiles of 32, not 48: that network halves three times and its depthwise stencil (tdr_dwsg_fwd) wants a width
that is a multiple of 4 at every level, 48 / 8 = 6 is refused (the note in test_hip_infer_session.py on its 32 x 96 image); 32 is the
next tile below that every level takes.  Images, overlap 16 and tile_batch 4 are unchanged."""
import os

import numpy as np
import pytest
import torch

import test_hip_infer_session as TS
import test_hip_sfnet_session as TSF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the bound of tests/test_hip_tile_kernels.py: at most 9 terms of two roundings each, 8 additions, weights summing to ~1
BLEND_ULPS = 16 * 2.0 ** -24


@pytest.fixture(autouse=True)
def bx3():
    from textualdegremoval_amd import kernels as K
    prev = K.MATH
    K.set_math('bx3')
    yield
    K.set_math(prev)


def _pair(tile):
    return (tile, tile) if isinstance(tile, int) else tile


def composite(net, lq, extra, tile, overlap, tile_batch):
    """-> (float64 [N,C,H,W], the map of pixels covered by one tile in both dimensions, max |tile output|); the forwards run eagerly under
    a session of their own (packed weights only: bit-identical to a replay, tests/test_hip_infer_session.py)"""
    from textualdegremoval_amd.inference import InferenceSession, full_size, tile_batches, tile_starts, tile_weights
    N, _, H, W = lq.shape
    (ys, th), (xs, tw) = tile_starts(H, _pair(tile)[0], overlap), tile_starts(W, _pair(tile)[1], overlap)
    x = lq.cpu().numpy()
    where = [(n, y0, x0) for n in range(N) for y0 in ys for x0 in xs]
    sess = InferenceSession(net, max_graphs=0)
    outs = {}
    for batch in tile_batches(len(where), tile_batch):
        assert len(batch) == tile_batch
        tiles = np.stack([x[n, :, y0:y0 + th, x0:x0 + tw] for n, y0, x0 in (where[i] for i in batch)])
        rows = torch.tensor([where[i][0] for i in batch], device='cuda')
        out = full_size(sess(torch.from_numpy(tiles).cuda(), *[e[rows] for e in extra])).cpu().numpy()
        for slot, i in enumerate(batch):
            outs.setdefault(i, out[slot])                                    # (a padding slot repeats a tile: the first one counts)
    sess.release()
    (fy, cy, wy), (fx, cx, wx) = tile_weights(H, _pair(tile)[0], overlap), tile_weights(W, _pair(tile)[1], overlap)
    want = np.zeros((N, outs[0].shape[0], H, W), np.float64)
    for i, (n, y0, x0) in enumerate(where):
        yy, xx = np.arange(y0, y0 + th), np.arange(x0, x0 + tw)
        iy, ix = ys.index(y0), xs.index(x0)
        w = wy[yy, iy - fy[yy]].astype(np.float64)[:, None] * wx[xx, ix - fx[xx]].astype(np.float64)[None, :]
        want[n, :, y0:y0 + th, x0:x0 + tw] += w * outs[i].astype(np.float64)
    once = (cy == 1)[:, None] & (cx == 1)[None, :]
    return want, once, max(np.abs(o).max() for o in outs.values())


def agrees(got, want, once, top):
    got = got.cpu().numpy()
    err = np.abs(got.astype(np.float64) - want).max()
    print(f'max |run_tiled - composite| {err:.3e}, bound {BLEND_ULPS * top:.3e} (max |tile output| {top:.3f}); '
          f'{once.mean():.2f} of the pixels covered once')
    assert got.shape == want.shape and err <= BLEND_ULPS * top
    assert np.array_equal(got[:, :, once].view(np.uint32), want.astype(np.float32)[:, :, once].view(np.uint32))


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def test_nafnet_w32_against_the_composite():
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    lq = _rand(1, 3, 80, 112, seed=21)
    sess = InferenceSession(net)
    got = sess.run_tiled(lq, tile=32, overlap=16, tile_batch=4)              # 4 x 6 tiles: six batches -- eager, capture + replay, 4 replays
    want, once, top = composite(net, lq, (), 32, 16, 4)
    assert once.any() and not once.all()
    agrees(got, want, once, top)
    assert sess.captures == 1 and sess.replays == 5
    zero = InferenceSession(net, max_graphs=0)                               # packed weights only: eager tile batches, the same bits
    assert torch.equal(zero.run_tiled(lq, tile=32, overlap=16, tile_batch=4), got) and zero.captures == 0
    agrees(zero.run_tiled(lq, tile=32, overlap=16, tile_batch=5), *composite(net, lq, (), 32, 16, 5))     # 24 tiles in fives: one padding slot
    for s in (sess, zero):
        s.release()
    with pytest.raises(RuntimeError):
        sess.run_tiled(lq, tile=32, overlap=16)


def test_one_tile_one_image_is_the_plain_call():
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    x = _rand(1, 3, 64, 64, seed=22)
    sess = InferenceSession(net)
    for _ in range(3):                                                       # eager, capture + replay, replay
        assert torch.equal(sess.run_tiled(x, tile=128, tile_batch=1), sess(x))
    assert len(sess.graphs) == 1                                             # ... of one and the same key
    sess.release()


def test_one_graph_for_every_image_size():
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    sess = InferenceSession(net)
    images = [_rand(1, 3, H, W, seed=23 + i) for i, (H, W) in enumerate(((80, 112), (96, 64), (70, 130)))]
    first = [sess.run_tiled(x, tile=32, overlap=16) for x in images]         # 24, 15 and 32 tiles: the 15 end in a padded batch
    assert all(o.shape == x.shape for o, x in zip(first, images))
    plans = list(sess.tile_plans.values())
    again = [sess.run_tiled(x, tile=32, overlap=16) for x in images]
    assert sess.captures == 1 and len(sess.graphs) == 1
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert len(plans) == 3 and all(p is q for p, q in zip(plans, sess.tile_plans.values()))      # the device tables were reused
    sess.release()
    assert not sess.tile_plans


def test_two_images_in_one_call():
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    lq = _rand(2, 3, 64, 80, seed=27)
    sess = InferenceSession(net)
    got = sess.run_tiled(lq, tile=32, overlap=16, tile_batch=4)              # 3 x 4 tiles per image: no batch mixes the two images
    for n in range(2):
        want, once, top = composite(net, lq[n:n + 1], (), 32, 16, 4)
        agrees(got[n:n + 1], want, once, top)
    sess.release()


def test_guided_network_ref_passed_whole():
    from textualdegremoval_amd.inference import InferenceSession
    net, (_, ref), _ = TS._guided('net_w8_128_wrap', None)
    ref = ref[:1].contiguous()
    kept = ref.clone()
    lq = _rand(1, 3, 160, 200, seed=28)
    sess = InferenceSession(net)
    got = sess.run_tiled(lq, ref, tile=128, overlap=32, tile_batch=4)
    want, once, top = composite(net, lq, (ref,), 128, 32, 4)
    agrees(got, want, once, top)
    assert torch.equal(ref, kept)
    sess.release()


def test_dynamic_fusion_k_v_as_the_extra():
    from textualdegremoval_amd.inference import InferenceSession
    net, (_, kv), _ = TS._dynfusion()
    lq = _rand(2, 3, 80, 112, seed=29)
    kv = kv[:2].contiguous()
    assert kv.shape == (2, 10, 1024) and not torch.equal(kv[0], kv[1])
    sess = InferenceSession(net)
    got = sess.run_tiled(lq, kv, tile=64, overlap=16, tile_batch=3)          # 4 tiles per image, 8 in batches of 3: images mix in a batch
    want, once, top = composite(net, lq, (kv,), 64, 16, 3)
    agrees(got, want, once, top)
    sess.release()


def test_sfnet_blends_the_full_size_output():
    from textualdegremoval_amd.inference import InferenceSession
    net = TSF.make_net(['train', 'Indoor']).eval()
    lq = _rand(1, 3, 48, 80, seed=30)
    sess = InferenceSession(net)
    assert [tuple(o.shape[2:]) for o in sess(lq[:, :, :32, :48].contiguous())] == [(8, 12), (16, 24), (32, 48)]
    got = sess.run_tiled(lq, tile=(32, 48), overlap=8, tile_batch=2)
    want, once, top = composite(net, lq, (), (32, 48), 8, 2)                 # (the composite blends full_size(out), the last of the list)
    assert got.shape == (1, 3, 48, 80)
    agrees(got, want, once, top)
    sess.release()


@pytest.mark.parametrize('bgr', [True, False])
def test_run_tiled_u8_is_the_byte_kernels_around_run_tiled(bgr):
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    u8 = torch.from_numpy(np.random.default_rng(31).integers(0, 256, size=(1, 80, 112, 3), dtype=np.uint8)).cuda()
    sess = InferenceSession(net)
    want = K.planes_to_img_u8(sess.run_tiled(K.img_u8_to_planes(u8, swap_rb=bgr), tile=32, overlap=16), swap_rb=bgr)
    captures = sess.captures
    got = sess.run_tiled_u8(u8, tile=32, overlap=16, bgr=bgr)
    assert got.dtype == torch.uint8 and got.shape == u8.shape and torch.equal(got, want)
    assert sess.captures == captures == 1 and len(sess.graphs) == 1          # the byte entry runs the float call's graph
    sess.release()


def test_run_tiled_u8_converts_a_byte_ref_once(monkeypatch):
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._guided('net_w8_128_wrap', None)
    rng = np.random.default_rng(32)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(1, 160, 200, 3), dtype=np.uint8)).cuda()
    ref = torch.from_numpy(rng.integers(0, 256, size=(1, 128, 128, 3), dtype=np.uint8)).cuda()
    sess = InferenceSession(net)
    want = K.planes_to_img_u8(sess.run_tiled(K.img_u8_to_planes(u8), K.img_u8_to_planes(ref), tile=128, overlap=32, tile_batch=2))
    calls, orig = [], K.img_u8_to_planes
    monkeypatch.setattr(K, 'img_u8_to_planes', lambda *a, **k: (calls.append(1), orig(*a, **k))[1])
    assert torch.equal(sess.run_tiled_u8(u8, ref, tile=128, overlap=32, tile_batch=2), want)
    assert len(calls) == 1                                                   # 4 tiles, 2 batches, one conversion of the ref
    sess.release()


def test_step_model_validates_tiled(monkeypatch, tmp_path):
    """`val: {tile, tile_overlap, tile_batch}` on the synthetic debug option file (window_size 8 stays: pad first, then tile): one
    nondist_validation over two images of different sizes reports the PSNR of run_tiled's output, from a single graph"""
    import torch.nn.functional as F
    from textualdegremoval_amd.metrics import calculate_psnr, tensor2img
    from textualdegremoval_amd.models import create_model
    from textualdegremoval_amd.utils.utils_options import parse
    monkeypatch.setenv('TDR_EXPERIMENTS_ROOT', str(tmp_path))
    opt = parse(os.path.join(ROOT, 'tests', 'data', 'train_nafnet_ref_synthetic_debug.yml'), is_train=True)
    opt['dist'] = False
    opt['val'].update(tile=48, tile_overlap=16, tile_batch=2)
    assert opt['val']['window_size'] == 8 and 'session' not in opt['val']
    model = create_model(opt)
    data = []
    for i, (H, W) in enumerate(((100, 76), (64, 120))):
        data.append({'lq': _rand(1, 3, H, W, seed=40 + i), 'gt': _rand(1, 3, H, W, seed=50 + i), 'ref': _rand(1, 3, 128, 128, seed=60 + i)})
    psnr = model.nondist_validation(data, 1, None, False, True, True)
    sessions = list(model._val_sessions.values())
    assert len(sessions) == 1 and sessions[0].captures == 1 and len(sessions[0].graphs) == 1
    assert model.output.shape == data[-1]['lq'].shape and model.net_g.training
    by_hand = []
    for d in data:
        H, W = d['lq'].shape[2:]
        padded = F.pad(d['lq'], (0, -W % 8, 0, -H % 8), 'reflect')
        out = sessions[0].run_tiled(padded, d['ref'], tile=48, overlap=16, tile_batch=2)[:, :, :H, :W]
        by_hand.append(calculate_psnr(tensor2img(out.cpu(), rgb2bgr=True), tensor2img(d['gt'].cpu(), rgb2bgr=True), crop_border=0,
                                      test_y_channel=False))
    assert psnr == model.metric_results['psnr'] == sum(by_hand) / 2
    assert sessions[0].captures == 1
