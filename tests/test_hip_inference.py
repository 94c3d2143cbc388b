"""The inference path of the NAFNet family: `with torch.no_grad(): net(lq, ref)` runs engine.net_fwd / unet_fwd with keep=False -- the
forward-only NAFBlock chains, nothing saved -- and must (1) give the bits of the grad-enabled forward, (2) keep nothing, (3) leave a
training run that validates between optimiser steps untouched and read the CURRENT weights, (4) not be slower than the training
forward.  Parity with the reference follows from (1) and the golden tests of test_hip_network.py / test_hip_unguided.py."""
import gc
import os
import statistics

import numpy as np
import pytest
import torch

from oracle import nafnet_ref_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
W8 = dict(width=8, nf=8, ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1, 1])
# the small golden shapes of test_hip_network.py: square (batch 2), zero-padded non-multiple, ref larger than lq (two encoder passes), the
# 128x128 wrap case, and the YAML widths (fusion blocks of 128 / 256 channels whose last block produces c_out = c / 2 rows in the fused tail)
GUIDED = [('net_w8_256_b2_clear', W8, None), ('net_w8_120x100_pad', W8, None), ('net_w8_256_ref384', W8, (384, 384)),
          ('net_w8_128_wrap', W8, None), ('net_w8_200x136_ref300', W8, (300, 300)),
          ('net_yaml_w64_128', dict(width=64, nf=64, enc_blk_nums=[1, 1, 1, 3], dec_blk_nums=[1, 1, 1, 1], middle_blk_num=1,
                                    ext_n_blocks=[4, 4, 4, 4], reffusion_n_blocks=[2, 2, 2, 2, 1]), None)]
# width 32, enc [1, 1, 1, 28] at 1 x 3 x 512 x 512: the headline network on a full test image
HEADLINE = dict(width=32, nf=32, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1], middle_blk_num=1, ext_n_blocks=[4, 4, 4, 4],
                reffusion_n_blocks=[2, 2, 2, 2, 2])


@pytest.fixture(params=['bx3', 'f32', 'hx2'])
def math_mode(request):
    from textualdegremoval_amd import kernels as K
    prev = K.MATH
    K.set_math(request.param)
    yield request.param
    K.set_math(prev)


def _guided_net(kw, seed):
    from textualdegremoval_amd.models.archs import define_network
    cfg = O.default_cfg(**kw)
    net = define_network(dict(type='NAFNetRefFusion', enc_blk_nums=cfg['enc_blk_nums'], dec_blk_nums=cfg['dec_blk_nums'],
                              middle_blk_num=cfg['middle_blk_num'], **{k: v for k, v in kw.items()
                                                                       if k not in ('enc_blk_nums', 'dec_blk_nums', 'middle_blk_num')}))
    net.load_state_dict(O.synth_params(cfg, seed=seed), strict=True)
    return net.cuda()


def _spy(monkeypatch, name):
    """records the `keep` every call of engine.<name> was made with"""
    from textualdegremoval_amd import engine as E
    orig, seen = getattr(E, name), []

    def wrapped(*a, **k):
        seen.append(k.get('keep', True))
        return orig(*a, **k)
    monkeypatch.setattr(E, name, wrapped)
    return seen


@pytest.mark.parametrize('name,kw,ref_hw', GUIDED)
def test_no_grad_forward_is_bit_identical_guided(math_mode, monkeypatch, name, kw, ref_hw):
    g = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    seed = int(g['seed'])
    net = _guided_net(kw, seed)
    lq, _, ref = O.synth_pair(int(g['cfg_B']), int(g['cfg_H']), int(g['cfg_W']), seed=1234 + seed, ref_hw=ref_hw)
    lq, ref = lq.cuda(), ref.cuda()
    seen = _spy(monkeypatch, 'net_fwd')
    out_train = net(lq, ref)                               # the grad-enabled forward: the autograd node, everything saved
    assert out_train.grad_fn is not None and seen == [True]
    with torch.no_grad():
        out = net(lq, ref)
    assert seen == [True, False] and not out.requires_grad
    assert torch.equal(out, out_train), (out - out_train).abs().max().item()
    net.eval()                                             # .eval() alone does not select the inference path ...
    assert net(lq, ref).grad_fn is not None and seen[-1] is True
    for p in net.parameters():                             # ... a forward nothing can ask a gradient of does
        p.requires_grad_(False)
    out2 = net(lq, ref)
    assert seen[-1] is False and out2.grad_fn is None and torch.equal(out2, out_train)
    out3 = net(lq.clone().requires_grad_(True), ref)       # (an input that requires grad: autograd again)
    assert seen[-1] is True and out3.requires_grad


@pytest.mark.parametrize('hw', [(44, 60), (64, 64)])
def test_no_grad_forward_is_bit_identical_unguided(math_mode, monkeypatch, hw):
    """`NAFNet` with the weights and the input of tests/golden/unguided.npz, (44 x 60: padded to 48 x 64), and a size the fused chains serve"""
    from textualdegremoval_amd.models.archs import define_network
    G = np.load(os.path.join(GOLDEN, 'unguided.npz'))
    net = define_network(dict(type='NAFNet', img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 2], dec_blk_nums=[1, 1, 1]))
    net.load_state_dict({str(k): torch.from_numpy(G[f'nafnet_p_{k}']) for k in G['nafnet_names']}, strict=True)
    net = net.cuda()
    x = torch.from_numpy(G['nafnet_x']).cuda()
    if tuple(x.shape[-2:]) != hw:
        x = torch.rand(2, 3, *hw, generator=torch.Generator().manual_seed(3)).cuda()
    seen = _spy(monkeypatch, 'unet_fwd')
    out_train = net(x)
    with torch.no_grad():
        out = net(x)
    assert seen == [True, False] and out_train.grad_fn is not None and not out.requires_grad
    assert torch.equal(out, out_train), (out - out_train).abs().max().item()
    # wide enough for the fused chains at every level (32 .. 256 channels), forward-only kernels against the training kernels
    net = define_network(dict(type='NAFNet', img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=[1, 1, 1], dec_blk_nums=[1, 1, 1]))
    torch.manual_seed(5)
    for k, p in net.named_parameters():
        if k.endswith(('beta', 'gamma')):
            torch.nn.init.normal_(p, std=0.3)
    net = net.cuda()
    out_train = net(x)
    with torch.no_grad():
        out = net(x)
    assert torch.equal(out, out_train), (out - out_train).abs().max().item()


def test_forward_only_blocks_bitwise_and_switch(math_mode):
    """engine.naf_fwd(keep=False) per channel count of the fused chains, and the two ways to the per-op launches (48 channels; 64 channels
    on 12 x 8 pixels, HW % 64 != 0 -- the depthwise stencil wants W % 4 == 0), full and c_out = c / 2: the bits of keep=True, nothing
    saved; engine.INFER_KERNELS = False (the probe's A/B) gives them too"""
    from textualdegremoval_amd import engine as E
    gen = torch.Generator().manual_seed(11)
    for c, hw in ((32, (16, 24)), (64, (16, 16)), (128, (8, 16)), (256, (8, 8)), (48, (16, 16)), (64, (12, 8))):
        P = {}
        for nm, shp in [('beta', (1, c, 1, 1)), ('gamma', (1, c, 1, 1)), ('conv1.weight', (2 * c, c, 1, 1)), ('conv1.bias', (2 * c,)),
                        ('conv2.weight', (2 * c, 1, 3, 3)), ('conv2.bias', (2 * c,)), ('conv3.weight', (c, c, 1, 1)), ('conv3.bias', (c,)),
                        ('sca.1.weight', (c, c, 1, 1)), ('sca.1.bias', (c,)), ('conv4.weight', (2 * c, c, 1, 1)), ('conv4.bias', (2 * c,)),
                        ('conv5.weight', (c, c, 1, 1)), ('conv5.bias', (c,)), ('norm1.weight', (c,)), ('norm1.bias', (c,)),
                        ('norm2.weight', (c,)), ('norm2.bias', (c,))]:
            P[nm] = (torch.randn(shp, generator=gen) * 0.2 + (1.0 if nm in ('norm1.weight', 'norm2.weight') else 0.0)).cuda()
        x = torch.randn(2, c, *hw, generator=gen).cuda()
        for c_out in (None, c // 2):
            want, saved = E.naf_fwd(x, P, c_out)
            assert saved is not None
            for kernels_on in (True, False):
                prev, E.INFER_KERNELS = E.INFER_KERNELS, kernels_on
                try:
                    got, none = E.naf_fwd(x, P, c_out, keep=False)
                finally:
                    E.INFER_KERNELS = prev
                assert none is None and torch.equal(got, want), (c, hw, c_out, kernels_on)


def _headline():
    net = _guided_net(HEADLINE, 7)
    lq, _, ref = O.synth_pair(1, 512, 512, seed=77)
    return net, lq.cuda(), ref.cuda()


def _peak_delta(fn):
    """torch.cuda.max_memory_allocated() above what was allocated before fn() ran, fn's result still alive at the end"""
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def test_nothing_kept_and_peak_memory_at_most_a_quarter():
    """width 32, enc [1, 1, 1, 28], 1 x 3 x 512 x 512.  A block keeps about 9 c-planes for its backward; over the 36 backbone blocks, the
    10 fusion blocks and the two MASA pyramids that is about 5.7 GB held until the call returns, against about 0.5 GB of pyramids,
    warped features, skips and one block's working set: a ratio of about 1 / 10 by count.  The bar is that count with a margin of
    2.5 x for allocator rounding and workspaces -- 1 / 4.  The no-grad forward is measured before the grad-enabled one (whatever scratch
    the process has not allocated yet counts against it) and once more after it."""
    from textualdegremoval_amd import engine as E
    net, lq, ref = _headline()

    def infer():
        with torch.no_grad():
            return net(lq, ref)
    first = _peak_delta(infer)
    train = _peak_delta(lambda: net(lq, ref))
    again = _peak_delta(infer)
    with torch.no_grad():
        out, saved = E.net_fwd({k: p.detach() for k, p in net.named_parameters()}, net.cfg, lq, ref, keep=False)
    assert saved is None
    del out
    print(f'peak memory above the resident state: no-grad forward {again / 2**20:.0f} MiB (first call {first / 2**20:.0f} MiB), '
          f'grad-enabled forward {train / 2**20:.0f} MiB, ratio {again / train:.4f} (first call {first / train:.4f})')
    assert again <= train / 4 and first <= train / 4, (first, again, train)


def test_no_grad_forward_is_not_slower():
    """same process, same shape, alternating runs, medians of device time (two events around a run of three forwards, so host jitter
    between a launch and its synchronise is not in the figure): the grad-enabled forward is the parent's code path, unchanged -- the
    forward that writes and allocates less must not take longer"""
    net, lq, ref = _headline()
    REP = 3

    def infer():
        with torch.no_grad():
            for _ in range(REP):
                net(lq, ref)

    def train():
        for _ in range(REP):
            net(lq, ref)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REP
    for fn in (train, infer, train, infer):                # warm-up: code objects, workspaces, allocator
        timed(fn)
    t_train, t_infer = [], []
    for _ in range(11):
        t_train.append(timed(train))
        t_infer.append(timed(infer))
    mt, mi = statistics.median(t_train), statistics.median(t_infer)
    print(f'forward at 1x3x512x512, width 32: grad-enabled median {mt:.2f} ms (min {min(t_train):.2f}), no-grad median {mi:.2f} ms '
          f'(min {min(t_infer):.2f})')
    assert mi <= mt, (t_infer, t_train)


def _trainer(seed):
    from textualdegremoval_amd.models import create_model
    model = create_model({
        'model_type': 'RefGuidedImageCleanModel', 'num_gpu': 1, 'dist': False, 'is_train': True,
        'network_g': dict(type='NAFNetRefFusion', enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1], middle_blk_num=1, **W8),
        'path': {},
        'train': {'optim_g': {'type': 'AdamW', 'lr': 2e-4, 'ref_lr': 1e-4, 'weight_decay': 1e-4, 'betas': [0.9, 0.999]},
                  'scheduler': {'type': 'CosineAnnealingRestartCyclicLR', 'periods': [30, 70], 'restart_weights': [1, 1],
                                'eta_mins': [3e-4, 1e-6]},
                  'pixel_opt': {'type': 'L1Loss', 'loss_weight': 1, 'reduction': 'mean'},
                  'use_grad_clip': True, 'total_iter': 100, 'warmup_iter': -1},
        'logger': {'check_freq': 10 ** 9}, 'val': {}, 'scale': 1})
    cfg = O.default_cfg(**W8)
    model.net_g.load_state_dict(O.synth_params(cfg, seed=seed), strict=True)
    return model


def test_validation_between_captured_steps(monkeypatch):
    """RefGuidedImageCleanModel with the hipGraph step (eager, eager, capture + replay, replay, replay): nonpad_test after steps 3 and 5
    reads the weights the optimiser has just written -- its output is the grad-enabled forward of the current parameters, bit for bit --
    and the loss trajectory is that of a run that never validated.  (kernels.DETERMINISTIC: the one order-dependent reduction of the step
    accumulates in fixed point, so two runs can be compared for equality.)"""
    from textualdegremoval_amd import kernels as K
    monkeypatch.setenv('TDR_GRAPH', '1')
    monkeypatch.setattr(K, 'DETERMINISTIC', True)
    lq, gt, ref = O.synth_pair(1, 128, 128, seed=1234 + 3)
    vlq, _, vref = O.synth_pair(1, 200, 136, seed=99, ref_hw=(300, 300))      # a validation image of another size than the step's

    def run(validate_after):
        model = _trainer(3)
        losses, vals = [], []
        for it in range(1, 6):
            model.update_learning_rate(it, warmup_iter=-1)
            model.feed_train_data({'lq': lq, 'gt': gt, 'ref': ref})
            model.optimize_parameters(it)
            losses.append(model.get_current_log()['l_pix'])
            if it in validate_after:
                for a, b in ((lq, ref), (vlq, vref)):
                    model.feed_data({'lq': a, 'ref': b})
                    model.nonpad_test()
                    assert not model.output.requires_grad and model.net_g.training
                    want = model.net_g(model.lq, model.ref)              # grad-enabled forward of the current parameters
                    assert want.grad_fn is not None
                    assert torch.equal(model.output, want.detach()), (it, (model.output - want).abs().max().item())
                    vals.append(model.output.clone())
        assert model._gstate['segs'] is not None                         # the step was captured and replayed
        return losses, vals
    plain, _ = run(())
    with_val, vals = run((3, 5))
    assert with_val == plain, (with_val, plain)
    assert len(vals) == 4 and not torch.equal(vals[0], vals[2])          # two more optimiser steps lie between the validations
