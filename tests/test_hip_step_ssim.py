"""SSIMLoss in the HIP train step (RefGuidedImageCleanModel): `train.ssim_opt` next to a pixel criterion and `pixel_opt: SSIMLoss` alone,
on the eager, surveyed and graph paths, under the default arithmetic (bx3) and the fp16 one (hx2).  The width-8 NAFNetRefFusion and the
1 x 3 x 128^2 synthetic pair of tests/test_hip_step.py."""
import math

import pytest
import torch

from oracle import nafnet_ref_oracle as O

pytestmark = pytest.mark.gpu

SSIM_W = 0.2


def make_opt(ssim_opt=True, pixel_opt=None):
    train = {'optim_g': {'type': 'AdamW', 'lr': 2e-4, 'ref_lr': 1e-4, 'weight_decay': 1e-4, 'betas': [0.9, 0.999]},
             'scheduler': {'type': 'CosineAnnealingRestartCyclicLR', 'periods': [30, 70], 'restart_weights': [1, 1],
                           'eta_mins': [3e-4, 1e-6]},
             'pixel_opt': pixel_opt or {'type': 'L1Loss', 'loss_weight': 1, 'reduction': 'mean'},
             'use_grad_clip': True, 'total_iter': 100, 'warmup_iter': -1}
    if ssim_opt:
        train['ssim_opt'] = {'type': 'SSIMLoss', 'loss_weight': SSIM_W}
    return {
        'model_type': 'RefGuidedImageCleanModel', 'num_gpu': 1, 'dist': False, 'is_train': True,
        'network_g': dict(type='NAFNetRefFusion', width=8, nf=8, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1],
                          middle_blk_num=1, ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1, 1]),
        'path': {}, 'train': train, 'logger': {'check_freq': 10 ** 9}, 'val': {}, 'scale': 1,
    }


def _model(**kw):
    from textualdegremoval_amd.models import create_model
    model = create_model(make_opt(**kw))
    cfg = O.default_cfg(width=8, nf=8, ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1, 1])
    model.net_g.load_state_dict(O.synth_params(cfg, seed=3), strict=True)
    return model


def _data():
    lq, gt, ref = O.synth_pair(1, 128, 128, seed=1234 + 3)
    return {'lq': lq, 'gt': gt, 'ref': ref}


def _step(model, it, data):
    model.update_learning_rate(it, warmup_iter=-1)
    model.feed_train_data(data)
    model.optimize_parameters(it)
    return model.get_current_log()


def _checksums(model):
    sd = model.net_g.state_dict()
    return [sd[k].double().sum().item() for k in sd]


def _criterion(model, data, weight=SSIM_W):
    from textualdegremoval_amd.losses import SSIMLoss
    return float(SSIMLoss(weight)(model.output, data['gt'].cuda()).item())


def _both_terms():
    """-> l_ssim of iteration 1.  Iterations 1 - 3 (eager, eager, capture + replay) and one more replay: after each step l_ssim is the
    criterion on that step's output bit for bit; iteration 1's l_pix is the pixel criterion alone with the bits of a model that has no
    ssim_opt; after three steps the structural term has moved the weights"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    data = _data()
    model, plain = _model(), _model(ssim_opt=False)
    first = None
    for it in range(1, 4):
        log, log_plain = _step(model, it, data), _step(plain, it, data)
        assert 'l_ssim' in log and 'l_ssim' not in log_plain
        assert math.isfinite(log['l_pix']) and math.isfinite(log['l_ssim'])
        assert log['l_ssim'] == _criterion(model, data), (it, log)
        if it == 1:
            first = log['l_ssim']
            assert log['l_pix'] == log_plain['l_pix'], (log, log_plain)
    assert any(a != b for a, b in zip(_checksums(model), _checksums(plain)))
    log = _step(model, 4, data)
    assert math.isfinite(log['l_pix']) and log['l_ssim'] == _criterion(model, data), log
    return first


_bx3 = {}


def _bx3_first_l_ssim():
    from textualdegremoval_amd import kernels as K
    if 'v' not in _bx3:
        prev = K.MATH
        K.set_math('bx3')
        try:
            model = _model()
            _bx3['v'] = _step(model, 1, _data())['l_ssim']
        finally:
            K.set_math(prev)
    return _bx3['v']


def test_ssim_opt_joins_the_step():
    from textualdegremoval_amd import kernels as K
    assert K.MATH == 'bx3'
    _bx3['v'] = _both_terms()


def test_ssim_opt_joins_the_step_hx2(hx2_mode):
    """the fp16 arithmetic: the first step is the range survey, the loss scale starts from max(lw_pix, 32 lw_ssim); l_ssim of
    iteration 1 within the project's SSIM bar (2e-4, times the weight) of the bx3 value"""
    first = _both_terms()
    assert math.isfinite(first) and abs(first - _bx3_first_l_ssim()) <= 2e-4 * SSIM_W


def test_ssim_loss_alone_as_pixel_opt():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    data = _data()
    model = _model(ssim_opt=False, pixel_opt={'type': 'SSIMLoss', 'loss_weight': 0.8})
    start = _checksums(model)
    for it in range(1, 4):
        log = _step(model, it, data)
        assert 'l_ssim' not in log
        assert math.isfinite(log['l_pix']) and log['l_pix'] == _criterion(model, data, 0.8), (it, log)
    assert any(a != b for a, b in zip(_checksums(model), start))
