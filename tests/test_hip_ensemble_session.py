"""InferenceSession.run_ensemble / run_ensemble_u8 / run_tiled(ensemble=) on the GPU against a composite built here from the definition
(inference.dihedral / dihedral_inverse): per class the transforms stacked op-major with ATen, one eager forward of the stack under a
session of its own (packed weights only), every answer transformed back, added in ascending op order in fp32 on the device, divided by
their number.  The composite uses the same batch composition as the call -- a sample's bits are not assumed independent of its
batch-mates.  Everything is compared with torch.equal."""
import os

import numpy as np
import pytest
import torch

import test_hip_infer_session as TS
import test_hip_sfnet_session as TSF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def bx3():
    from textualdegremoval_amd import kernels as K
    prev = K.MATH
    K.set_math('bx3')
    yield
    K.set_math(prev)


def _rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def composite(net, lq, extra, ops):
    from textualdegremoval_amd.inference import InferenceSession, dihedral, dihedral_inverse, ensemble_ops, full_size
    sel = ensemble_ops(ops)
    sess = InferenceSession(net, max_graphs=0)
    N, s = lq.shape[0], None
    for cls in (tuple(k for k in sel if k < 4), tuple(k for k in sel if k >= 4)):
        if not cls:
            continue
        images = [torch.cat([dihedral(lq, op).contiguous() for op in cls])]
        for e in extra:
            images.append(torch.cat([dihedral(e, op).contiguous() for op in cls]) if e.dim() == 4 else e.repeat(len(cls), *([1] * (e.dim() - 1))))
        out = full_size(sess(*images))
        for i, op in enumerate(cls):
            v = dihedral_inverse(out[i * N:(i + 1) * N], op).contiguous()
            s = v if s is None else s + v
    sess.release()
    return s / torch.tensor(float(len(sel)), dtype=torch.float32, device=s.device)


def test_nafnet_w32_non_square_two_keys():
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    x = _rand(1, 3, 32, 64, seed=71)
    kept = x.clone()
    sess = InferenceSession(net)
    first = sess.run_ensemble(x)
    assert first.shape == x.shape and torch.equal(first, composite(net, x, (), 8))
    assert sess.captures == 0 and sorted(k[0][0][0] for k in sess.warm) == [(4, 3, 32, 64), (4, 3, 64, 32)]      # two keys, both warm
    assert torch.equal(sess.run_ensemble(x), first)                          # both classes capture + replay
    assert sess.captures == 2 and sess.replays == 2
    assert torch.equal(sess.run_ensemble(x), first)                          # two replays
    assert sess.captures == 2 and sess.replays == 4 and len(sess.graphs) == 2
    assert torch.equal(x, kept)
    sess.release()
    with pytest.raises(RuntimeError):
        sess.run_ensemble(x)


def test_nafnet_w32_square_one_key_and_the_smaller_selections():
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    x = _rand(1, 3, 32, 32, seed=72)
    sess = InferenceSession(net)
    first = sess.run_ensemble(x)                                             # straight class eager, transposed class: the same key, captured
    assert sess.captures == 1 and len(sess.graphs) == 1 and len(sess.warm) == 1
    assert torch.equal(first, composite(net, x, (), 8))
    assert torch.equal(sess.run_ensemble(x), first) and sess.captures == 1
    assert torch.equal(sess.run_ensemble(x, ops=4), composite(net, x, (), 4))
    assert torch.equal(sess.run_ensemble(x, ops=(0, 5)), composite(net, x, (), (0, 5)))
    assert torch.equal(sess.run_ensemble(x, ops=(6, 1, 0, 6)), composite(net, x, (), (0, 1, 6)))      # three members: a division by 3.0f
    assert torch.equal(sess.run_ensemble(x, ops=1), sess(x))
    assert not torch.equal(sess.run_ensemble(x, ops=1), first)               # (the ensemble is not the plain forward)
    with pytest.raises(ValueError):
        sess.run_ensemble(x, ops=3)
    with pytest.raises(TypeError):
        sess.run_ensemble(x.double())
    sess.release()


def test_guided_network_transforms_the_ref_with_its_image():
    from textualdegremoval_amd.inference import InferenceSession
    net, (lq, ref), _ = TS._guided('net_w8_128_wrap', None)
    lq, ref = lq[:1].contiguous(), ref[:1].contiguous()
    kept = ref.clone()
    sess = InferenceSession(net)
    got = sess.run_ensemble(lq, ref)
    assert got.shape == lq.shape and torch.equal(got, composite(net, lq, (ref,), 8))
    assert torch.equal(ref, kept)
    sess.release()


def test_dynamic_fusion_repeats_k_v_op_major():
    from textualdegremoval_amd.inference import InferenceSession
    net, (lq, kv), _ = TS._dynfusion()
    lq, kv = lq[:2, :, :32, :].contiguous(), kv[:2].contiguous()
    assert lq.shape == (2, 3, 32, 64) and kv.shape == (2, 10, 1024) and not torch.equal(kv[0], kv[1])
    sess = InferenceSession(net)
    got = sess.run_ensemble(lq, kv)
    assert torch.equal(got, composite(net, lq, (kv,), 8))
    assert torch.equal(sess.run_ensemble(lq, kv), got) and sess.captures == 2
    with pytest.raises(NotImplementedError, match='16 images'):
        sess.run_ensemble(torch.cat([lq, lq, lq]).contiguous(), torch.cat([kv, kv, kv]).contiguous(), ops=4)      # 24 images: the network's own limit
    sess.release()


def test_sfnet_averages_the_full_size_output():
    from textualdegremoval_amd.inference import InferenceSession
    net = TSF.make_net(['train', 'Indoor']).eval()
    lq = _rand(1, 3, 32, 48, seed=75)
    sess = InferenceSession(net)
    got = sess.run_ensemble(lq)
    assert got.shape == (1, 3, 32, 48) and torch.equal(got, composite(net, lq, (), 8))
    assert torch.equal(sess.run_ensemble(lq), got) and sess.captures == 2
    sess.release()


@pytest.mark.parametrize('bgr', [True, False])
def test_run_ensemble_u8_is_the_byte_kernels_around_run_ensemble(bgr):
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    u8 = torch.from_numpy(np.random.default_rng(76).integers(0, 256, size=(1, 32, 64, 3), dtype=np.uint8)).cuda()
    sess = InferenceSession(net)
    planes = K.img_u8_to_planes(u8, swap_rb=bgr)
    want = K.planes_to_img_u8(sess.run_ensemble(planes), swap_rb=bgr)
    assert torch.equal(K.planes_to_img_u8(sess.run_ensemble(planes), swap_rb=bgr), want)      # (warm, then captured: the same bits)
    captures, keys = sess.captures, sess.graphs.keys()
    assert captures == 2
    got = sess.run_ensemble_u8(u8, bgr=bgr)
    assert got.dtype == torch.uint8 and got.shape == u8.shape and torch.equal(got, want)
    assert sess.captures == captures and sess.graphs.keys() == keys          # the byte entry replays the float call's graphs
    assert sess.replays == 4
    with pytest.raises(TypeError):
        sess.run_ensemble_u8(planes)
    sess.release()


def test_run_ensemble_u8_gathers_a_byte_ref():
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._guided('net_w8_128_wrap', None)
    rng = np.random.default_rng(77)
    u8 = torch.from_numpy(rng.integers(0, 256, size=(1, 128, 128, 3), dtype=np.uint8)).cuda()
    ref = torch.from_numpy(rng.integers(0, 256, size=(1, 128, 128, 3), dtype=np.uint8)).cuda()
    sess = InferenceSession(net)
    want = K.planes_to_img_u8(sess.run_ensemble(K.img_u8_to_planes(u8), K.img_u8_to_planes(ref), ops=(0, 3, 5)))
    assert torch.equal(sess.run_ensemble_u8(u8, ref, ops=(0, 3, 5)), want)
    sess.release()


def test_tiled_ensemble_is_the_mean_of_two_tiled_runs():
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.inference import InferenceSession
    net, _, _ = TS._nafnet_w32()
    lq = _rand(1, 3, 80, 112, seed=78)
    sess = InferenceSession(net)
    kw = dict(tile=32, overlap=16, tile_batch=4)
    got = sess.run_tiled(lq, ensemble=8, **kw)
    assert sess.captures == 1 and len(sess.graphs) == 1                      # square tiles: one graph for both classes
    straight = sess.run_tiled(K.dihedral_gather(lq, (0, 1, 2, 3)), **kw)
    transposed = sess.run_tiled(K.dihedral_gather(lq, (4, 5, 6, 7)), **kw)
    assert straight.shape == (4, 3, 80, 112) and transposed.shape == (4, 3, 112, 80)
    assert got.shape == lq.shape and torch.equal(got, K.dihedral_mean(straight, transposed, tuple(range(8)), 1))
    assert sess.captures == 1 and len(sess.graphs) == 1
    # non-square tiles: (th, tw) for the straight class, (tw, th) for the transposed one
    kw2 = dict(tile=(32, 64), overlap=16, tile_batch=4)
    want = K.dihedral_mean(sess.run_tiled(K.dihedral_gather(lq, (1,)), **kw2),
                           sess.run_tiled(K.dihedral_gather(lq, (6,)), tile=(64, 32), overlap=16, tile_batch=4), (1, 6), 1)
    assert torch.equal(sess.run_tiled(lq, ensemble=(1, 6), **kw2), want)
    # bytes: the byte kernels around the float call
    u8 = torch.from_numpy(np.random.default_rng(79).integers(0, 256, size=(1, 80, 112, 3), dtype=np.uint8)).cuda()
    for bgr in (True, False):
        want = K.planes_to_img_u8(sess.run_tiled(K.img_u8_to_planes(u8, swap_rb=bgr), ensemble=8, **kw), swap_rb=bgr)
        got_u8 = sess.run_tiled_u8(u8, ensemble=8, bgr=bgr, **kw)
        assert got_u8.dtype == torch.uint8 and torch.equal(got_u8, want)
    # without the keyword nothing changes
    assert torch.equal(sess.run_tiled(lq, ensemble=None, **kw), sess.run_tiled(lq, **kw))
    assert torch.equal(sess.run_tiled_u8(u8, ensemble=None, **kw), sess.run_tiled_u8(u8, **kw))
    assert torch.equal(sess.run_tiled(lq, ensemble=1, **kw), sess.run_tiled(lq, **kw))      # (one member, divided by 1.0f)
    with pytest.raises(NotImplementedError):
        sess.run_tiled(lq, lq, matcher=object(), ensemble=8, **kw)
    with pytest.raises(NotImplementedError):
        sess.run_tiled_u8(u8, u8, matcher=object(), ensemble=8, **kw)
    sess.release()


def _debug_opt(monkeypatch, tmp_path, **val):
    from textualdegremoval_amd.utils.utils_options import parse
    monkeypatch.setenv('TDR_EXPERIMENTS_ROOT', str(tmp_path))
    opt = parse(os.path.join(ROOT, 'tests', 'data', 'train_nafnet_ref_synthetic_debug.yml'), is_train=True)
    opt['dist'] = False
    opt['val'].update(**val)
    assert opt['val']['window_size'] == 8 and 'session' not in opt['val']
    return opt


def _psnr(out, gt):
    from textualdegremoval_amd.metrics import calculate_psnr, tensor2img
    return calculate_psnr(tensor2img(out.cpu(), rgb2bgr=True), tensor2img(gt.cpu(), rgb2bgr=True), crop_border=0, test_y_channel=False)


def test_step_model_validates_with_the_ensemble(monkeypatch, tmp_path):
    """`val: {ensemble: 8}` on the synthetic debug option file (window_size 8 stays: pad first): with val.tile through run_tiled -- two
    images of different sizes, one session, one capture; without it through run_ensemble; with val.tile_match a ValueError"""
    import torch.nn.functional as F
    from textualdegremoval_amd.models import create_model
    model = create_model(_debug_opt(monkeypatch, tmp_path, tile=48, tile_overlap=16, tile_batch=2, ensemble=8))
    data = []
    for i, (H, W) in enumerate(((100, 76), (64, 120))):
        data.append({'lq': _rand(1, 3, H, W, seed=80 + i), 'gt': _rand(1, 3, H, W, seed=90 + i), 'ref': _rand(1, 3, 128, 128, seed=100 + i)})
    psnr = model.nondist_validation(data, 1, None, False, True, True)
    sessions = list(model._val_sessions.values())
    assert len(sessions) == 1 and sessions[0].captures == 1 and len(sessions[0].graphs) == 1
    assert model.output.shape == data[-1]['lq'].shape and model.net_g.training
    by_hand, plain = [], []
    for d in data:
        H, W = d['lq'].shape[2:]
        padded = F.pad(d['lq'], (0, -W % 8, 0, -H % 8), 'reflect')
        out = sessions[0].run_tiled(padded, d['ref'], tile=48, overlap=16, tile_batch=2, ensemble=8)[:, :, :H, :W]
        by_hand.append(_psnr(out, d['gt']))
        plain.append(_psnr(sessions[0].run_tiled(padded, d['ref'], tile=48, overlap=16, tile_batch=2)[:, :, :H, :W], d['gt']))
    assert psnr == model.metric_results['psnr'] == sum(by_hand) / 2
    assert psnr != sum(plain) / 2                                            # (not the validation without the key)
    assert sessions[0].captures == 1

    model = create_model(_debug_opt(monkeypatch, tmp_path, ensemble=8))      # no tiles: run_ensemble on the padded image
    d = {'lq': _rand(1, 3, 128, 128, seed=110), 'gt': _rand(1, 3, 128, 128, seed=111), 'ref': _rand(1, 3, 128, 128, seed=112)}
    psnr = model.nondist_validation([d], 1, None, False, True, True)
    sessions = list(model._val_sessions.values())
    assert len(sessions) == 1
    assert psnr == _psnr(sessions[0].run_ensemble(d['lq'], d['ref'], ops=8), d['gt'])
    assert psnr != _psnr(sessions[0](d['lq'], d['ref']), d['gt'])

    model = create_model(_debug_opt(monkeypatch, tmp_path, tile=48, tile_match=True, ensemble=8))
    with pytest.raises(ValueError, match='ensemble'):
        model.nonpad_test(d['lq'])
