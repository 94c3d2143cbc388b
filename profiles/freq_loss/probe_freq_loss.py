"""FFTLoss on the device (csrc/tdr_freq_loss.hip), one process, one GPU.  No pass bar.
  launches: at 4x3x512^2, 4x3x256^2 and 1x3x128^2, REPS calls captured into one hipGraph, events around a replay, over REPS -- device time
    of one call without the host's launch cost: kernels.freq_loss value only (table, rows, columns forward + partial sums, finish), value +
    gradient (the columns also inverse and written back, rows back), two-sided and one-sided; beside it kernels.pixel_loss(L1) and the
    project's copy kernel (kernels.dihedral_gather, op 0: one plane pass in, one out), whose rate makes the floor: 7 plane passes with the
    gradient (pred, target, workspace out, workspace in and out, workspace in, dpred out), 3 for the value alone; and the same criterion as
    torch.fft under ATen autograd on the device, forward + backward, eager, events around REPS calls (or the error, if this torch build
    has no FFT backend on the device).
  per-launch split: `--trace N --shape I` runs nothing but N eager value + gradient calls of shape I after a warm-up, for
    `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python ... --trace N --shape I`; `--stats DIR0,DIR1,DIR2` then reads the
    kernel rows of those three runs into the JSON; `--pmc DIR`: the counter rows of a `rocprofv3 --pmc SQ_LDS_BANK_CONFLICT ...` run of
    `--trace N --shape 0`, taken on its own, per kernel and dispatch (the column pass runs below half the floor rate).
  step: optimize_parameters of the headline configuration (NAFNetRefFusion width 32, enc [1, 1, 1, 28], batch 4, 512^2, bx3, graph
    replay) called through the model with and without `freq_opt: {type: FFTLoss, loss_weight: 0.1}`: warm steps (eager, eager, capture),
    then `--rounds` alternating a / b, wall time between two device synchronisations, medians, and the a-to-a spread between even and
    odd rounds as the noise floor.
  loss scale: under hx2, the width-8 test network at 1x3x128^2 and the headline batch: the exponent the step starts from
    (max(lw_pix, 4 sqrt(H W) lw_freq) in the formula of _fwd_bwd) and what the first-step range survey made of it, with and without freq_opt.
Synthetic weights: no restoration-quality figure.
Writes profiles/freq_loss/probe_freq_loss.json (or `--out PATH`).   python profiles/freq_loss/probe_freq_loss.py [--out PATH] [--rounds R]"""
import argparse
import csv
import glob
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

import _freq_loss_ref as R  # noqa: E402
from oracle import nafnet_ref_oracle as O  # noqa: E402
from textualdegremoval_amd import _lib  # noqa: E402
from textualdegremoval_amd import kernels as K  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'freq_loss', 'probe_freq_loss.json'))
ap.add_argument('--rounds', type=int, default=9)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--skip-step', action='store_true')
ap.add_argument('--trace', type=int, default=0)
ap.add_argument('--shape', type=int, default=0)
ap.add_argument('--stats', default='')
ap.add_argument('--pmc', default='')
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_freq_loss.py measures on the GPU'
K.set_math('bx3')
SHAPES = ((4, 3, 512, 512), (4, 3, 256, 256), (1, 3, 128, 128))
HEADLINE = dict(width=32, nf=32, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1], middle_blk_num=1, ext_n_blocks=[4, 4, 4, 4],
                reffusion_n_blocks=[2, 2, 2, 2, 2])
SMALL = dict(width=8, nf=8, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1], middle_blk_num=1, ext_n_blocks=[1, 1, 1, 1],
             reffusion_n_blocks=[1, 1, 1, 1, 1])
FREQ_W = 0.1

if a.trace:
    pred, gt = (t.cuda() for t in R.make_inputs(SHAPES[a.shape], SHAPES[a.shape][2]))
    for _ in range(3 + a.trace):
        K.freq_loss(pred, gt, FREQ_W)
    torch.cuda.synchronize()
    sys.exit(0)


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


def kernel_rows(directory):
    """the freq_* rows of a rocprofv3 --stats csv directory: kernel -> (calls, average ns)"""
    rows = {}
    for path in glob.glob(os.path.join(directory, '**', '*kernel_stats.csv'), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get('Name', '')
                if 'freq_' in name:
                    short = name[name.index('freq_'):].split('(')[0].split('E')[0]
                    rows[short] = dict(calls=int(r['Calls']), average_us=round(float(r['AverageNs']) / 1e3, 2))
    return rows


def counter_rows(directory):
    """the freq_* rows of a rocprofv3 --pmc csv directory: kernel -> counter -> mean value per dispatch"""
    acc = {}
    for path in glob.glob(os.path.join(directory, '**', '*counter_collection.csv'), recursive=True):
        with open(path) as f:
            for r in csv.DictReader(f):
                name = r.get('Kernel_Name', '')
                if 'freq_' in name:
                    short = name[name.index('freq_'):].split('(')[0].split('E')[0]
                    acc.setdefault(short, {}).setdefault(r['Counter_Name'], []).append(float(r['Counter_Value']))
    return {k: {c: dict(dispatches=len(v), mean=round(sum(v) / len(v), 1)) for c, v in cs.items()} for k, cs in acc.items()}


def model_for(net_kw, freq_opt):
    from textualdegremoval_amd.models import create_model
    cfg = O.default_cfg(**net_kw)
    net = dict(type='NAFNetRefFusion', enc_blk_nums=cfg['enc_blk_nums'], dec_blk_nums=cfg['dec_blk_nums'], middle_blk_num=cfg['middle_blk_num'],
               **{k: v for k, v in net_kw.items() if k not in ('enc_blk_nums', 'dec_blk_nums', 'middle_blk_num')})
    train = {'optim_g': {'type': 'AdamW', 'lr': 2e-4, 'ref_lr': 1e-4, 'weight_decay': 1e-4, 'betas': [0.9, 0.999]},
             'scheduler': {'type': 'CosineAnnealingRestartCyclicLR', 'periods': [30, 70], 'restart_weights': [1, 1], 'eta_mins': [3e-4, 1e-6]},
             'pixel_opt': {'type': 'L1Loss', 'loss_weight': 1, 'reduction': 'mean'}, 'use_grad_clip': True, 'total_iter': 100, 'warmup_iter': -1}
    if freq_opt:
        train['freq_opt'] = {'type': 'FFTLoss', 'loss_weight': FREQ_W}
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


res = dict(probe='freq_loss', device=torch.cuda.get_device_name(0), rounds=a.rounds, reps=a.reps,
           note='launches: device microseconds of one call (hipGraph of `reps` calls / reps); floor: 7 (3) plane passes at the rate of the '
                'copy kernel; step: wall milliseconds of optimize_parameters',
           launches={}, loss_scale={}, step={})
stat_dirs = a.stats.split(',') if a.stats else []
if a.pmc:
    res['lds_bank_conflict'] = dict(shape='x'.join(map(str, SHAPES[0])), counters=counter_rows(a.pmc),
                                    note='rocprofv3 --pmc, a run of its own; mean per dispatch of each kernel')

for i, shape in enumerate(SHAPES):
    pred, gt = (t.cuda() for t in R.make_inputs(shape, shape[2]))
    plane_bytes = pred.numel() * 4
    row = dict(freq_loss_value_only_us=graph_us(lambda: K.freq_loss(pred, gt, FREQ_W, want_grad=False)),
               freq_loss_value_and_grad_us=graph_us(lambda: K.freq_loss(pred, gt, FREQ_W)),
               freq_loss_onesided_value_and_grad_us=graph_us(lambda: K.freq_loss(pred, gt, FREQ_W, True)),
               pixel_loss_l1_us=graph_us(lambda: K.pixel_loss(K.LOSS_L1, pred, gt, 1.0, 0.0)),
               copy_kernel_us=graph_us(lambda: K.dihedral_gather(pred, [0])),
               plane_bytes=plane_bytes, ws_bytes=int(_lib.load().tdr_freq_loss_ws_bytes(*shape)))
    row['copy_rate_TBps'] = round(2 * plane_bytes / row['copy_kernel_us'] / 1e6, 3)
    row['floor_value_and_grad_us'] = round(3.5 * row['copy_kernel_us'], 1)
    row['floor_value_only_us'] = round(1.5 * row['copy_kernel_us'], 1)
    row['value_and_grad_over_floor'] = round(row['freq_loss_value_and_grad_us'] / row['floor_value_and_grad_us'], 2)
    row['value_only_over_floor'] = round(row['freq_loss_value_only_us'] / row['floor_value_only_us'], 2)
    if i < len(stat_dirs):
        row['per_launch_rocprofv3'] = kernel_rows(stat_dirs[i])

    def aten():
        p = pred.clone().requires_grad_(True)
        R.literal(p, gt, FREQ_W).backward()
        return p.grad
    try:
        aten()
        row['aten_autograd_fwd_bwd_eager_us'] = eager_us(aten)
    except Exception as e:                       # no FFT backend in this torch build: recorded instead of a number
        row['aten_autograd_fwd_bwd_eager_us'] = None
        row['aten_error'] = f'{type(e).__name__}: {str(e)[:200]}'
    res['launches']['x'.join(map(str, shape))] = row
    save(res)

# the loss scale of the fp16 arithmetic: the starting exponent and what the first survey made of it
K.set_math('hx2')
try:
    for name, net_kw, batch, size in (('width8_1x3x128x128', SMALL, 1, 128), ('headline_4x3x512x512', HEADLINE, 4, 512)):
        lq, gt, ref = O.synth_pair(batch, size, size, seed=1234)
        data = {'lq': lq, 'gt': gt, 'ref': ref}
        for label, freq_opt in (('l1_alone', False), ('l1_plus_freq', True)):
            model = model_for(net_kw, freq_opt)
            rows = []
            for it in (1, 2, 3):
                step(model, it, data)
                g = model.optimizer_g.guard.read()
                r = getattr(model, 'last_range_survey', None)
                rows.append(dict(iter=it, last_survey_iter=getattr(model, '_last_survey_iter', None),
                                 scale_exponent_after=round(math.log2(g.scale), 2),
                                 scale_shift_total=getattr(model, '_scale_shift', 0), skipped=int(g.skipped),
                                 grad_window_log2=list(r['grad']) if r else None, math=K.MATH,
                                 bwd_full_range=bool(getattr(model, '_bwd_full_range', False)), log=model.get_current_log()))
            res['loss_scale'][f'{name}/{label}'] = dict(start_exponent=round(math.log2(model.loss_scale_start), 2), steps=rows)
            del model
            torch.cuda.empty_cache()
            K.set_math('hx2')
            save(res)
finally:
    K.set_math('bx3')

if not a.skip_step:
    lq, gt, ref = O.synth_pair(4, 512, 512, seed=1234)
    data = {'lq': lq, 'gt': gt, 'ref': ref}
    models = {'a_l1_alone': model_for(HEADLINE, False), 'b_l1_plus_freq': model_for(HEADLINE, True)}
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
    ta, tb = ts['a_l1_alone'], ts['b_l1_plus_freq']
    res['step']['headline_4x3x512x512_bx3'] = dict(
        ms={k: stats(v) for k, v in ts.items()}, a_to_a_spread_ms=round(abs(statistics.median(ta[0::2]) - statistics.median(ta[1::2])), 3),
        freq_term_cost_ms=round(statistics.median(tb) - statistics.median(ta), 3),
        logs={k: m.get_current_log() for k, m in models.items()})
    save(res)
print(json.dumps(res))
