"""FFTLoss in the HIP train step (RefGuidedImageCleanModel): `train.freq_opt` next to a pixel criterion (and next to `ssim_opt`) and
`pixel_opt: FFTLoss` alone, on the eager, surveyed and graph paths, under the default arithmetic (bx3) and the fp16 one (hx2).  The width-8
NAFNetRefFusion and the 1 x 3 x 128^2 synthetic pair of tests/test_hip_step.py."""
import math

import pytest
import torch

from oracle import nafnet_ref_oracle as O

pytestmark = pytest.mark.gpu

FREQ_W = 0.1
SSIM_W = 0.2


def make_opt(freq_opt=True, ssim_opt=False, pixel_opt=None):
    train = {'optim_g': {'type': 'AdamW', 'lr': 2e-4, 'ref_lr': 1e-4, 'weight_decay': 1e-4, 'betas': [0.9, 0.999]},
             'scheduler': {'type': 'CosineAnnealingRestartCyclicLR', 'periods': [30, 70], 'restart_weights': [1, 1],
                           'eta_mins': [3e-4, 1e-6]},
             'pixel_opt': pixel_opt or {'type': 'L1Loss', 'loss_weight': 1, 'reduction': 'mean'},
             'use_grad_clip': True, 'total_iter': 100, 'warmup_iter': -1}
    if freq_opt:
        train['freq_opt'] = {'type': 'FFTLoss', 'loss_weight': FREQ_W}
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


def _data(size=128):
    lq, gt, ref = O.synth_pair(1, size, size, seed=1234 + 3)
    return {'lq': lq, 'gt': gt, 'ref': ref}


def _step(model, it, data):
    model.update_learning_rate(it, warmup_iter=-1)
    model.feed_train_data(data)
    model.optimize_parameters(it)
    return model.get_current_log()


def _checksums(model):
    sd = model.net_g.state_dict()
    return [sd[k].double().sum().item() for k in sd]


def _freq(model, data, weight=FREQ_W):
    from textualdegremoval_amd.losses import FFTLoss
    return float(FFTLoss(weight)(model.output, data['gt'].cuda()).item())


def _ssim(model, data):
    from textualdegremoval_amd.losses import SSIMLoss
    return float(SSIMLoss(SSIM_W)(model.output, data['gt'].cuda()).item())


def _both_terms():
    """iterations 1 - 3 (eager, eager, capture + replay) and one more replay: after each step l_freq is the criterion on that step's output
    bit for bit; iteration 1's l_pix has the bits of a model without freq_opt; after three steps the term has moved the weights"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    data = _data()
    model, plain = _model(), _model(freq_opt=False)
    for it in range(1, 4):
        log, log_plain = _step(model, it, data), _step(plain, it, data)
        assert 'l_freq' in log and 'l_freq' not in log_plain and 'l_ssim' not in log
        assert math.isfinite(log['l_pix']) and math.isfinite(log['l_freq'])
        assert log['l_freq'] == _freq(model, data), (it, log)
        if it == 1:
            assert log['l_pix'] == log_plain['l_pix'], (log, log_plain)
    assert any(a != b for a, b in zip(_checksums(model), _checksums(plain)))
    log = _step(model, 4, data)
    assert math.isfinite(log['l_pix']) and log['l_freq'] == _freq(model, data), log
    return model


def test_freq_opt_joins_the_step():
    from textualdegremoval_amd import kernels as K
    assert K.MATH == 'bx3'
    _both_terms()


def test_freq_opt_joins_the_step_hx2(hx2_mode):
    """the fp16 arithmetic: the first step is the range survey, the loss scale starts from max(lw_pix, 4 sqrt(H W) lw_freq) = 51.2 here"""
    model = _both_terms()
    guard = model.optimizer_g.guard.read()
    start = math.log2(model.loss_scale_start)
    assert start == math.floor(math.log2(512.0 * 1 * 3 * 128 * 128 / (4.0 * 128 * FREQ_W)))      # 4 sqrt(H W) lw_freq = 51.2 > lw_pix
    survey = getattr(model, 'last_range_survey', None)
    print(f'hx2: loss scale started at 2^{start:.0f}, shift after the surveys {getattr(model, "_scale_shift", 0)}, now 2^{math.log2(guard.scale):.0f}; '
          f'grad window of the last survey {survey["grad"] if survey else None}; skipped steps {model.skipped_steps}')
    assert math.isfinite(guard.scale) and guard.scale > 0


def test_fft_loss_alone_as_pixel_opt():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    data = _data()
    model = _model(freq_opt=False, pixel_opt={'type': 'FFTLoss', 'loss_weight': 0.8})
    start = _checksums(model)
    for it in range(1, 4):
        log = _step(model, it, data)
        assert 'l_freq' not in log and 'l_ssim' not in log
        assert math.isfinite(log['l_pix']) and log['l_pix'] == _freq(model, data, 0.8), (it, log)
    assert any(a != b for a, b in zip(_checksums(model), start))


def test_freq_opt_and_ssim_opt_together():
    """all three log entries, each the criterion on the step's output bit for bit (eager, eager, capture + replay), and the dpred the
    backward pass starts from is the sum of the three terms in the order pixel -> ssim -> freq"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.losses import L1Loss
    data = _data()
    model = _model(ssim_opt=True)
    seen = {}
    eng = getattr(model.get_bare_model(model.net_g), 'engine', None)
    if eng is None:
        from textualdegremoval_amd import engine as eng
    real = eng.net_bwd

    def spy(dpred, *a, **kw):
        seen['dpred'] = dpred.clone()
        return real(dpred, *a, **kw)
    eng.net_bwd = spy
    try:
        log = _step(model, 1, data)
    finally:
        eng.net_bwd = real
    gt = data['gt'].cuda()
    out = model.output.contiguous()
    _, want = K.pixel_loss(K.LOSS_L1, out, gt, 1.0, 0.0)
    _, _, want = K.ssim_loss(out, gt, SSIM_W, 1.0, dpred=want)
    _, want = K.freq_loss(out, gt, FREQ_W, False, dpred=want)
    assert torch.equal(seen['dpred'], want)
    for it in range(1, 4):
        if it > 1:
            log = _step(model, it, data)
        assert set(log) >= {'l_pix', 'l_ssim', 'l_freq'}
        assert log['l_freq'] == _freq(model, data) and log['l_ssim'] == _ssim(model, data), (it, log)
        assert log['l_pix'] == float(L1Loss()(model.output, gt).item()), (it, log)


def test_inadmissible_size_raises_value_error():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    model = _model()
    data = _data()
    data = {k: v[..., :100, :100].contiguous() for k, v in data.items()}
    model.update_learning_rate(1, warmup_iter=-1)
    model.feed_train_data(data)
    with pytest.raises(ValueError, match='100 x 100'):
        model.optimize_parameters(1)
