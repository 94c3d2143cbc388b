"""SSIMLoss on the device (csrc/tdr_ssim_loss.hip), one process, one GPU.  No pass bar.
  launches: at 4x3x512^2, 4x3x256^2 and 1x3x128^2, REPS calls captured into one hipGraph, events around a replay, over REPS -- device time
    of one call without the host's launch cost: kernels.ssim_loss value only (forward + finish), value + gradient (forward writing the
    coefficient maps, finish, the gather backward: form a, the one form built), kernels.pixel_loss(L1) beside it, and the same torch
    expression (tests/_ssim_loss_ref.py) under ATen autograd on the device, forward + backward, eager, events around REPS calls.
  step: optimize_parameters of the headline configuration (NAFNetRefFusion width 32, enc [1, 1, 1, 28], batch 4, 512^2, bx3, graph
    replay) called through the model with and without `ssim_opt: {type: SSIMLoss, loss_weight: 0.2}`: warm steps (eager, eager, capture),
    then `--rounds` alternating a / b, wall time between two device synchronisations, medians, and the a-to-a spread between even and
    odd rounds as the noise floor.
  loss scale: under hx2, the width-8 test network at 1x3x128^2 and the headline batch: the exponent the step starts from
    (max(lw_pix, 32 lw_ssim) in the formula of _fwd_bwd) and what the first-step range survey made of it, with and without ssim_opt.
Synthetic weights: no restoration-quality figure.
Writes profiles/ssim_loss/probe_ssim_loss.json (or `--out PATH`).   python profiles/ssim_loss/probe_ssim_loss.py [--out PATH] [--rounds R]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import _ssim_loss_ref as R  # noqa: E402
from oracle import nafnet_ref_oracle as O  # noqa: E402
from textualdegremoval_amd import _lib  # noqa: E402
from textualdegremoval_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssim_loss', 'probe_ssim_loss.json'))
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--skip-step', action='store_true')
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_ssim_loss.py measures on the GPU'
K.set_math('bx3')
SHAPES = ((4, 3, 512, 512), (4, 3, 256, 256), (1, 3, 128, 128))
HEADLINE = dict(width=32, nf=32, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1], middle_blk_num=1, ext_n_blocks=[4, 4, 4, 4],
                reffusion_n_blocks=[2, 2, 2, 2, 2])
SMALL = dict(width=8, nf=8, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1], middle_blk_num=1, ext_n_blocks=[1, 1, 1, 1],
             reffusion_n_blocks=[1, 1, 1, 1, 1])
SSIM_W = 0.2


def save(res):
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


def stats(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def graph_us(fn):
    fn()
    torch.cuda.synchronize()
    g, keep = torch.cuda.CUDAGraph(), []
    with torch.cuda.graph(g):
        for _ in range(a.reps):
            keep.append(fn())
    ts = []
    for _ in range(a.rounds + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    del g, keep
    return round(statistics.median(ts[2:]), 1)


def eager_us(fn):
    ts = []
    for _ in range(a.rounds + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3 / a.reps)
    return round(statistics.median(ts[2:]), 1)


def model_for(net_kw, ssim_opt):
    from textualdegremoval_amd.models import create_model
    cfg = O.default_cfg(**net_kw)
    net = dict(type='NAFNetRefFusion', enc_blk_nums=cfg['enc_blk_nums'], dec_blk_nums=cfg['dec_blk_nums'], middle_blk_num=cfg['middle_blk_num'],
               **{k: v for k, v in net_kw.items() if k not in ('enc_blk_nums', 'dec_blk_nums', 'middle_blk_num')})
    train = {'optim_g': {'type': 'AdamW', 'lr': 2e-4, 'ref_lr': 1e-4, 'weight_decay': 1e-4, 'betas': [0.9, 0.999]},
             'scheduler': {'type': 'CosineAnnealingRestartCyclicLR', 'periods': [30, 70], 'restart_weights': [1, 1], 'eta_mins': [3e-4, 1e-6]},
             'pixel_opt': {'type': 'L1Loss', 'loss_weight': 1, 'reduction': 'mean'}, 'use_grad_clip': True, 'total_iter': 100, 'warmup_iter': -1}
    if ssim_opt:
        train['ssim_opt'] = {'type': 'SSIMLoss', 'loss_weight': SSIM_W}
    model = create_model({'model_type': 'RefGuidedImageCleanModel', 'num_gpu': 1, 'dist': False, 'is_train': True, 'network_g': net,
                          'path': {}, 'train': train, 'logger': {'check_freq': 10 ** 9}, 'val': {}, 'scale': 1})
    model.net_g.load_state_dict(O.synth_params(cfg, seed=7), strict=True)
    return model


def step(model, it, data):
    model.update_learning_rate(it, warmup_iter=-1)
    model.feed_train_data(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.optimize_parameters(it)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


res = dict(probe='ssim_loss', device=torch.cuda.get_device_name(0), rounds=a.rounds, reps=a.reps, backward_form='a (coefficient maps + gather)',
           note='launches: device microseconds of one call (hipGraph of `reps` calls / reps); step: wall milliseconds of optimize_parameters',
           launches={}, loss_scale={}, step={})

for shape in SHAPES:
    pred, gt = (t.cuda() for t in R.make_inputs(shape, 'noise', 1.0, seed=shape[2]))
    row = dict(ssim_loss_value_only_us=graph_us(lambda: K.ssim_loss(pred, gt, SSIM_W, want_grad=False)),
               ssim_loss_value_and_grad_us=graph_us(lambda: K.ssim_loss(pred, gt, SSIM_W)),
               pixel_loss_l1_us=graph_us(lambda: K.pixel_loss(K.LOSS_L1, pred, gt, 1.0, 0.0)),
               ws_bytes=int(_lib.load().tdr_ssim_loss_ws_bytes(*shape)))
    row['ssim_loss_backward_us'] = round(row['ssim_loss_value_and_grad_us'] - row['ssim_loss_value_only_us'], 1)

    def aten():
        p = pred.clone().requires_grad_(True)
        R.ssim_loss(p, gt, SSIM_W, 1.0)[0].backward()
        return p.grad
    aten()
    row['aten_autograd_fwd_bwd_eager_us'] = eager_us(aten)
    res['launches']['x'.join(map(str, shape))] = row
    save(res)

# the loss scale of the fp16 arithmetic: the starting exponent and what the first survey made of it
K.set_math('hx2')
try:
    for name, net_kw, batch, size in (('width8_1x3x128x128', SMALL, 1, 128), ('headline_4x3x512x512', HEADLINE, 4, 512)):
        lq, gt, ref = O.synth_pair(batch, size, size, seed=1234)
        data = {'lq': lq, 'gt': gt, 'ref': ref}
        for label, ssim_opt in (('l1_alone', False), ('l1_plus_ssim', True)):
            model = model_for(net_kw, ssim_opt)
            rows = []
            for it in (1, 2, 3):
                step(model, it, data)
                g = model.optimizer_g.guard.read()
                r = getattr(model, 'last_range_survey', None)
                # (_last_survey_iter: the iteration of the last survey that found nothing to correct; None: the next step surveys again)
                rows.append(dict(iter=it, last_survey_iter=getattr(model, '_last_survey_iter', None),
                                 scale_exponent_after=round(math.log2(g.scale), 2),
                                 scale_shift_total=getattr(model, '_scale_shift', 0), skipped=int(g.skipped),
                                 grad_window_log2=list(r['grad']) if r else None, math=K.MATH,
                                 bwd_full_range=bool(getattr(model, '_bwd_full_range', False)), log=model.get_current_log()))
            lw_scale = max(1.0, 32 * SSIM_W) if ssim_opt else 1.0
            res['loss_scale'][f'{name}/{label}'] = dict(start_exponent=math.floor(math.log2(512.0 * batch * 3 * size * size / lw_scale)), steps=rows)
            del model
            torch.cuda.empty_cache()
            K.set_math('hx2')
            save(res)
finally:
    K.set_math('bx3')

if not a.skip_step:
    lq, gt, ref = O.synth_pair(4, 512, 512, seed=1234)
    data = {'lq': lq, 'gt': gt, 'ref': ref}
    models = {'a_l1_alone': model_for(HEADLINE, False), 'b_l1_plus_ssim': model_for(HEADLINE, True)}
    it = {k: 0 for k in models}
    ts = {k: [] for k in models}
    for k, m in models.items():
        for _ in range(5):                      # eager, eager, capture + replay, replays
            it[k] += 1
            step(m, it[k], data)
    for _ in range(a.rounds):
        for k, m in models.items():
            it[k] += 1
            ts[k].append(step(m, it[k], data))
    ta, tb = ts['a_l1_alone'], ts['b_l1_plus_ssim']
    res['step']['headline_4x3x512x512_bx3'] = dict(
        ms={k: stats(v) for k, v in ts.items()}, a_to_a_spread_ms=round(abs(statistics.median(ta[0::2]) - statistics.median(ta[1::2])), 3),
        ssim_term_cost_ms=round(statistics.median(tb) - statistics.median(ta), 3),
        logs={k: m.get_current_log() for k, m in models.items()})
    save(res)
print(json.dumps(res))
