"""Validation metrics on the device (csrc/tdr_valmetrics.hip through kernels.val_metrics, metrics.device and the step model's
`val: {device_metrics: true}`) against the host path they replace: tensor2img, then metrics.calculate_psnr / calculate_ssim.

The image domain is bytes, so the bars are bits wherever the host path is itself exact or runs the same kernel arithmetic:
  S / max / count     the numpy integers, exactly
  PSNR                calculate_psnr's float64, bit for bit
  SSIM (3-D window)   calculate_ssim's value, bit for bit (K.ssim3d on the same bytes, the per-image max_value rule included), and within
                      2e-4 of oracle.metrics_oracle.calculate_ssim, the bar of tests/test_hip_psnr_parity.py
  Y planes            metrics.to_y_channel's float32 bits, every pixel (all 2^24 colours in one 4096 x 4096 image)
  SSIM-Y              calculate_ssim(test_y_channel=True)'s float64, bit for bit (K.ssim_y64 on the same planes)
  PSNR-Y              the squared-error sum within 1e-9 relative of the float64 sum over the same planes (at most 2^20 addends rounded
                      at 2^-53 each: 1.2e-10 in the worst case); the dB within 1e-3 of calculate_psnr(test_y_channel=True), which
                      evaluates that branch in float32 -- the project's PSNR bar
Shapes are the smallest that take every clamp and tail: odd sizes, a whole tile, an image shorter than the 11-tap window, several
tiles and images; crops 0 and 4, and 12 on 37 x 53 (13 x 29 left: less than a tile)."""
import os
import struct

import numpy as np
import pytest
import torch

import _val_metrics_ref as VR

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ALL = ('psnr', 'ssim', 'psnr_y', 'ssim_y')
CASES = [((1, 3, 37, 53), 0), ((1, 3, 37, 53), 4), ((1, 3, 37, 53), 12), ((2, 3, 16, 16), 0), ((2, 3, 16, 16), 4),
         ((1, 1, 11, 70), 0), ((1, 1, 11, 70), 4), ((3, 3, 64, 48), 0), ((3, 3, 64, 48), 4)]


def _bits(x):
    return struct.pack('<d', float(x))


def _pair(shape, seed, form):
    """pred / gt on the host in one of the two forms: 'f' float32 [N,C,H,W] reaching past [0, 1], 'u' uint8 [N,H,W,C]"""
    N, C, H, W = shape
    rng = np.random.default_rng(seed)
    if form == 'u':
        a = rng.integers(0, 256, (N, H, W, C), dtype=np.uint8)
        return torch.from_numpy(a)
    return torch.from_numpy((rng.random((N, C, H, W), dtype=np.float32) * 1.2 - 0.1).astype(np.float32))


def _near(t, seed):
    """a ground truth a few grey levels away from t, same form"""
    rng = np.random.default_rng(seed)
    if t.dtype == torch.uint8:
        return torch.from_numpy(np.clip(t.numpy().astype(np.int64) + rng.integers(-9, 10, t.shape), 0, 255).astype(np.uint8))
    return t + torch.from_numpy(rng.normal(0, 0.03, t.shape).astype(np.float32))


def _host_img(t, n, swap):
    """image n as the validation loop hands it to the metrics: tensor2img of a float tensor, the bytes themselves otherwise"""
    from textualdegremoval_amd.metrics import tensor2img
    if t.dtype == torch.uint8:
        img = t[n].numpy()
        return img[:, :, 0] if img.shape[2] == 1 else img
    return tensor2img(t[n:n + 1], rgb2bgr=swap)


def _check_against_host(pred, gt, crop, swap, dev_pred=None, dev_gt=None, oracle='f32'):
    """every column of val_metrics, and metrics.device on top of it, against the host path -- image by image.  oracle: 'f32' the float32
    conv3d of oracle.metrics_oracle, 'f64' the float64 restatement of tests/_val_metrics_ref.py"""
    from oracle import metrics_oracle as MO
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd import metrics as M
    from textualdegremoval_amd.metrics.device import ValMetrics, _psnr_finish
    dp = pred.cuda() if dev_pred is None else dev_pred
    dg = gt.cuda() if dev_gt is None else dev_gt
    rows, ya, yb = K.val_metrics(dp, dg, crop_border=crop, swap_rb=swap, what=ALL, want_y=True)
    rows2, ya2, _ = K.val_metrics(dp, dg, crop_border=crop, swap_rb=swap, what=ALL, want_y=True)
    assert torch.equal(rows.view(torch.int64), rows2.view(torch.int64)) and torch.equal(ya.view(torch.int32), ya2.view(torch.int32))
    rows, ya, yb = rows.cpu().numpy(), ya.cpu().numpy(), yb.cpu().numpy()
    want_rows, want_ya, want_yb = VR.rows(pred, gt, crop, swap, want_y=True)
    N, C = rows.shape[0], (pred.shape[3] if pred.dtype == torch.uint8 else pred.shape[1])
    spec = {'psnr': {'type': 'calculate_psnr', 'crop_border': crop, 'test_y_channel': False},
            'ssim': {'type': 'calculate_ssim', 'crop_border': crop, 'test_y_channel': False},
            'psnr_y': {'type': 'calculate_psnr', 'crop_border': crop, 'test_y_channel': True},
            'ssim_y': {'type': 'calculate_ssim', 'crop_border': crop, 'test_y_channel': True}}
    vm = ValMetrics(spec)
    vm.add(dp, dg, rgb2bgr=swap)
    means = vm.result()
    host = {m: 0 for m in spec}
    for n in range(N):
        a, b = _host_img(pred, n, swap), _host_img(gt, n, swap)
        for c in ('S', 'MAX', 'COUNT', 'COUNT_Y'):
            assert rows[n, VR.COLS[c]] == want_rows[n, VR.COLS[c]], (n, c, rows[n], want_rows[n])
        psnr = M.calculate_psnr(a, b, crop)
        assert _bits(_psnr_finish(rows[n], False, C)) == _bits(psnr) == _bits(vm.per_image['psnr'][n]), (n, rows[n], psnr)
        ssim = M.calculate_ssim(a, b, crop)
        assert _bits(rows[n, VR.COLS['SSIM3D']]) == _bits(ssim) == _bits(vm.per_image['ssim'][n]), (n, rows[n, 3], ssim)
        ca = (a if a.ndim == 3 else a[..., None])[crop:a.shape[0] - crop, crop:a.shape[1] - crop]
        cb = (b if b.ndim == 3 else b[..., None])[crop:b.shape[0] - crop, crop:b.shape[1] - crop]
        want = MO.calculate_ssim(a, b, crop) if oracle == 'f32' else VR.ssim3d_f64(ca, cb, 1 if ca.max() <= 1 else 255)
        assert abs(ssim - want) < 2e-4 and abs(rows[n, VR.COLS['SSIM3D']] - want) < 2e-4, (n, rows[n, 3], want)
        # Y planes: to_y_channel of the cropped host images, every pixel
        hy_a, hy_b = M.to_y_channel(ca.astype(np.float64))[..., 0], M.to_y_channel(cb.astype(np.float64))[..., 0]
        assert np.array_equal(ya[n].view(np.uint32), hy_a.view(np.uint32)) and np.array_equal(yb[n].view(np.uint32), hy_b.view(np.uint32))
        assert np.array_equal(ya[n].view(np.uint32), want_ya[n].view(np.uint32))
        ssim_y = M.calculate_ssim(a, b, crop, test_y_channel=True)
        assert _bits(rows[n, VR.COLS['SSIMY']]) == _bits(ssim_y) == _bits(vm.per_image['ssim_y'][n]), (n, rows[n, 6], ssim_y)
        sy = want_rows[n, VR.COLS['SY']]
        assert abs(rows[n, VR.COLS['SY']] - sy) <= 1e-9 * sy, (n, rows[n, VR.COLS['SY']], sy)
        psnr_y = M.calculate_psnr(a, b, crop, test_y_channel=True)
        assert abs(vm.per_image['psnr_y'][n] - psnr_y) < 1e-3, (n, vm.per_image['psnr_y'][n], psnr_y)
        for m, v in (('psnr', psnr), ('ssim', ssim), ('ssim_y', ssim_y)):
            host[m] += v
    for m in ('psnr', 'ssim', 'ssim_y'):
        assert _bits(means[m]) == _bits(host[m] / N), (m, means[m], host[m] / N)
    return rows


@pytest.mark.parametrize('shape,crop', CASES)
def test_every_column_against_the_host_path(shape, crop):
    seed = 1000 + shape[2] * 7 + crop
    for forms in ('uu', 'ff', 'fu'):
        pred = _pair(shape, seed, forms[0])
        # (mixed forms: a byte ground truth a few levels off the float pred's own quantisation)
        gt = _near(pred if forms[0] == forms[1] else torch.from_numpy(VR.quantise(pred, False)), seed + 1)
        for swap in (False, True):
            _check_against_host(pred, gt, crop, swap)


def test_padded_strides_go_in_as_they_are():
    base_p, base_g = _pair((1, 3, 40, 56), 5, 'f'), _pair((1, 3, 40, 56), 6, 'f')
    dp, dg = base_p.cuda()[:, :, :37, :53], base_g.cuda()[:, :, :37, :53]
    assert not dp.is_contiguous()
    rows = _check_against_host(base_p[:, :, :37, :53], base_g[:, :, :37, :53], 4, True, dev_pred=dp, dev_gt=dg)
    assert rows[0, VR.COLS['COUNT']] == 29 * 45 * 3


def test_identical_unit_and_smooth_images():
    from textualdegremoval_amd.metrics.device import psnr_ssim
    rng = np.random.default_rng(21)
    u = torch.from_numpy(rng.integers(0, 256, (1, 37, 53, 3), dtype=np.uint8))
    p, s = psnr_ssim(u.cuda(), u.cuda())
    assert p == float('inf') and s == 1.0
    f = _pair((1, 3, 37, 53), 22, 'f')
    assert psnr_ssim(f.cuda(), f.clone().cuda(), crop_border=4)[0] == float('inf')
    # every byte <= 1: max_value 1 in both metrics, per image -- the second image of the batch is an ordinary one
    unit = torch.from_numpy(rng.integers(0, 2, (2, 37, 53, 3), dtype=np.uint8))
    unit[1] = u[0]
    gt = unit.clone()
    gt[0] ^= torch.from_numpy(rng.integers(0, 2, (37, 53, 3), dtype=np.uint8))
    gt[1] = _near(u, 23)[0]
    rows = _check_against_host(unit, gt, 0, True)
    assert rows[0, VR.COLS['MAX']] == 1 and rows[1, VR.COLS['MAX']] > 1
    # smooth: constant 200 +- 1 -- variances of order 1 under means of order 200, carried by the tile-centre shift
    a = torch.from_numpy((200 + rng.integers(-1, 2, (1, 64, 48, 3))).astype(np.uint8))
    b = torch.from_numpy((200 + rng.integers(-1, 2, (1, 64, 48, 3))).astype(np.uint8))
    # (the float32 conv3d of oracle.metrics_oracle loses exactly these variances -- 0.97915 where float64 gives 0.97814 and the kernels
    # 0.97814 -- so the 2e-4 bar is taken against the float64 evaluation here)
    _check_against_host(a, b, 0, True, oracle='f64')
    _check_against_host(a, b, 4, False, oracle='f64')


def test_quantisation_edges_are_planes_to_img_u8s():
    """k/255 +- 1 ulp, the ties (k + 1/2)/255, values below 0 and above 1: the Y plane of a 1-channel source is float32(u)/255*255, so
    y_pred pins every byte, and S against zeros their squares -- both against K.planes_to_img_u8 on the same planes"""
    from textualdegremoval_amd import kernels as K
    k = np.arange(256, dtype=np.float32)
    base = (k / np.float32(255)).astype(np.float32)
    ties = ((k.astype(np.float64) + 0.5) / 255).astype(np.float32)
    vals = np.concatenate([base, np.nextafter(base, np.float32(2)), np.nextafter(base, np.float32(-1)), ties,
                           np.nextafter(ties, np.float32(2)), np.nextafter(ties, np.float32(-1)),
                           np.array([-1.0, -1e-8, -0.0, 1.0000001, 2.0, 1e30, -1e30], np.float32)])
    H, W = 23, 71
    x = torch.from_numpy(np.resize(vals, H * W).astype(np.float32).reshape(1, 1, H, W)).cuda()
    want = K.planes_to_img_u8(x)[0, :, :, 0].cpu().numpy()
    rows, ya, _ = K.val_metrics(x, torch.zeros_like(x), what=('psnr', 'psnr_y'), want_y=True)
    rows = rows.cpu().numpy()
    assert np.array_equal(ya[0].cpu().numpy().view(np.uint32), (VR.LUT[want] * np.float32(255.)).view(np.uint32))
    assert len(np.unique(want)) == 256
    assert rows[0, 0] == (want.astype(np.int64) ** 2).sum() and rows[0, 1] == 255 and rows[0, 2] == H * W


@pytest.fixture(scope='module')
def all_colours():
    from textualdegremoval_amd.metrics import to_y_channel
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(1, 4096, 4096, 3)
    return img, to_y_channel(img[0].astype(np.float64))[..., 0]


def test_y_plane_of_all_colours(all_colours):
    """one launch over a 4096 x 4096 byte image holding every colour once, Y only; bytes are taken as they are under both swap_rb"""
    from textualdegremoval_amd import kernels as K
    img, want = all_colours
    d = torch.from_numpy(img).cuda()
    for swap in (False, True):
        rows, ya, yb = K.val_metrics(d, d, swap_rb=swap, what=('y',))
        assert np.array_equal(ya[0].cpu().numpy().view(np.uint32), want.view(np.uint32))
        assert torch.equal(ya, yb)
        rows = rows.cpu().numpy()
        assert rows[0, 0] == 0 and rows[0, 1] == 255 and rows[0, 2] == 3 * (1 << 24) and rows[0, 4] == 0 and rows[0, 5] == 1 << 24
    # a float source holding the same colours (k / 255 quantises back to k): swap_rb exchanges what the coefficients meet
    part = torch.from_numpy(img[:, :64]).cuda()
    planes = K.img_u8_to_planes(part, swap_rb=False)
    _, ya, _ = K.val_metrics(planes, planes, swap_rb=False, what=('y',))
    assert np.array_equal(ya[0].cpu().numpy().view(np.uint32), want[:64].view(np.uint32))
    _, ya, _ = K.val_metrics(planes, planes, swap_rb=True, what=('y',))
    assert np.array_equal(ya[0].cpu().numpy().view(np.uint32), VR.y_plane(np.ascontiguousarray(img[0, :64, :, ::-1])).view(np.uint32))


def test_a_batch_equals_its_images_one_by_one():
    from textualdegremoval_amd import kernels as K
    pred = _pair((3, 3, 64, 48), 31, 'f').cuda()
    gt = _near(_pair((3, 3, 64, 48), 31, 'f'), 32).cuda()
    rows, ya, yb = K.val_metrics(pred, gt, crop_border=4, what=ALL, want_y=True)
    for n in range(3):
        r1, a1, b1 = K.val_metrics(pred[n:n + 1], gt[n:n + 1], crop_border=4, what=ALL, want_y=True)
        assert torch.equal(r1[0].view(torch.int64), rows[n].view(torch.int64))
        assert torch.equal(a1[0], ya[n]) and torch.equal(b1[0], yb[n])


def test_refusals_raise():
    from textualdegremoval_amd import _lib
    from textualdegremoval_amd import kernels as K
    x = torch.zeros(1, 2, 8, 8, device='cuda')
    with pytest.raises(_lib.TdrError, match='channels'):
        K.val_metrics(x, x)
    x = torch.zeros(1, 3, 8, 12, device='cuda')
    with pytest.raises(_lib.TdrError, match='crop'):
        K.val_metrics(x, x, crop_border=4)
    with pytest.raises(ValueError):
        K.val_metrics(x, x, what=('niqe',))
    with pytest.raises(ValueError):
        K.val_metrics(x, torch.zeros(1, 3, 8, 8, device='cuda'))


# ---- the step model ----------------------------------------------------------------------------------------------------------------
def _model_and_data(**val):
    from oracle import nafnet_ref_oracle as NO
    from textualdegremoval_amd.models import create_model
    g = np.load(os.path.join(GOLDEN, 'net_w8_256_b2.npz'), allow_pickle=False)
    seed = int(g['seed'])
    cfg = NO.default_cfg(width=8, nf=8, ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1, 1])
    net = dict(type='NAFNetRefFusion', width=cfg['width'], nf=cfg['nf'], enc_blk_nums=cfg['enc_blk_nums'],
               dec_blk_nums=cfg['dec_blk_nums'], middle_blk_num=cfg['middle_blk_num'], ext_n_blocks=cfg['ext_n_blocks'],
               reffusion_n_blocks=cfg['reffusion_n_blocks'])
    opt = {     # (the option block of tests/test_hip_psnr_parity.py, PSNR + SSIM in val.metrics)
        'model_type': 'RefGuidedImageCleanModel', 'num_gpu': 1, 'dist': False, 'is_train': True, 'network_g': net, 'path': {},
        'train': {'optim_g': {'type': 'AdamW', 'lr': 2e-4, 'ref_lr': 1e-4, 'weight_decay': 1e-4, 'betas': [0.9, 0.999]},
                  'scheduler': {'type': 'CosineAnnealingRestartCyclicLR', 'periods': [30, 70], 'restart_weights': [1, 1],
                                'eta_mins': [3e-4, 1e-6]},
                  'pixel_opt': {'type': 'L1Loss', 'loss_weight': 1, 'reduction': 'mean'},
                  'use_grad_clip': True, 'total_iter': 100, 'warmup_iter': -1},
        'logger': {'check_freq': 10 ** 9}, 'scale': 1,
        'val': {'metrics': {'psnr': {'type': 'calculate_psnr', 'crop_border': 0, 'test_y_channel': False},
                            'ssim': {'type': 'calculate_ssim', 'crop_border': 0, 'test_y_channel': False}}},
    }
    opt['val'].update(val)
    model = create_model(opt)
    model.net_g.load_state_dict(NO.synth_params(cfg, seed=seed), strict=True)
    lq, gt, ref = NO.synth_pair(int(g['cfg_B']), int(g['cfg_H']), int(g['cfg_W']), seed=1234 + seed)
    return model, [{'lq': lq[b:b + 1], 'gt': gt[b:b + 1], 'ref': ref[b:b + 1]} for b in range(lq.shape[0])]


@pytest.mark.parametrize('val', [{}, {'session': True}, {'window_size': 48}], ids=['plain', 'session', 'window48'])
def test_step_model_reports_the_same_metric_results(val, monkeypatch):
    model, data = _model_and_data(**val)
    assert len(data) == 2
    last_host = model.validation(data, 0, None, save_img=False, rgb2bgr=True, use_image=True)
    host = dict(model.metric_results)
    if 'window_size' in val:
        assert tuple(model.output.shape[2:]) == (256, 256) and not model.output.is_contiguous()     # the padded, sliced output
    model.opt['val']['device_metrics'] = True

    def never(self=None):
        raise AssertionError('get_current_visuals reached with val.device_metrics')
    monkeypatch.setattr(model, 'get_current_visuals', never)
    last_dev = model.validation(data, 0, None, save_img=False, rgb2bgr=True, use_image=True)
    dev = dict(model.metric_results)
    assert list(dev) == list(host) == ['psnr', 'ssim']
    for m in host:
        assert _bits(dev[m]) == _bits(host[m]), (m, dev[m], host[m])
    assert _bits(last_dev) == _bits(last_host)


def test_step_model_refusals():
    model, data = _model_and_data(device_metrics=True)
    with pytest.raises(ValueError, match='use_image'):
        model.validation(data, 0, None, save_img=False, rgb2bgr=True, use_image=False)
    with pytest.raises(ValueError, match='gt'):
        model.validation([{k: v for k, v in data[0].items() if k != 'gt'}], 0, None, save_img=False, rgb2bgr=True, use_image=True)
    model.opt['val']['metrics']['niqe'] = {'type': 'calculate_niqe', 'crop_border': 0}
    with pytest.raises(ValueError, match='calculate_niqe'):
        model.validation(data, 0, None, save_img=False, rgb2bgr=True, use_image=True)
