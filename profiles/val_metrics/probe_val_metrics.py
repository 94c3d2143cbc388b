"""Validation with and without `val: {device_metrics: true}` (csrc/tdr_valmetrics.hip), one process, one GPU, bx3.  No pass bar.
  validation: the headline NAFNetRefFusion (width 32, enc [1, 1, 1, 28]) as a step model with `val: {session: true}` and PSNR + SSIM in
    val.metrics, a list of 8 images (lq, gt and ref of one size, host tensors as a loader hands them over) at 256 x 256 and at 720 x 1280.
    Wall time of model.validation(...) between two device synchronisations, a: the host loop (get_current_visuals, tensor2img,
    calculate_psnr, calculate_ssim per image), b: device_metrics; two warm validations each (the session captures its graph in the
    first), then `--rounds` alternating a / b, medians, and the a-to-a spread between the even and the odd rounds as the noise floor.
    The two report the same numbers bit for bit (asserted).  Device-to-host reads (Tensor.cpu / .item / .tolist on a device tensor) are
    counted per validation by wrapping those three methods.
  kernels: kernels.val_metrics(pred, gt, what=('psnr', 'ssim')) on float32 1 x 3 x H x W, REPS calls captured into one hipGraph, events
    around a replay, over REPS: device time of one call (its 5 launches) without the host's launch cost; and the wall time of the host
    path on the same image (tensor2img x 2, calculate_psnr, calculate_ssim), which includes its three copies and K.ssim3d.
  `--trace N`: nothing but N eager val_metrics calls per size after a warm-up, for `rocprofv3 --kernel-trace --stats -- python ... --trace N`;
    the per-kernel rows of that run are stored next to the JSON (kernel_stats_rocprofv3.csv).
No restoration-quality figure: the network carries synthetic weights.
Writes profiles/val_metrics/probe_val_metrics.json (or `--out PATH`).   python profiles/val_metrics/probe_val_metrics.py [--out PATH] [--rounds R]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import test_hip_inference as TI  # noqa: E402
from oracle import nafnet_ref_oracle as O  # noqa: E402
from textualdegremoval_amd import kernels as K  # noqa: E402
from textualdegremoval_amd import metrics as M  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'val_metrics', 'probe_val_metrics.json'))
ap.add_argument('--rounds', type=int, default=7)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--images', type=int, default=8)
ap.add_argument('--trace', type=int, default=0)
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_val_metrics.py measures on the GPU'
K.set_math('bx3')
SIZES = ((256, 256), (720, 1280))


def pair(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, 3, H, W, generator=g) * 1.1 - 0.05
    return x, (x + 0.03 * torch.randn(1, 3, H, W, generator=g))


if a.trace:
    for H, W in SIZES:
        p, g = (t.cuda() for t in pair(H, W, H))
        for _ in range(3 + a.trace):
            K.val_metrics(p, g, what=('psnr', 'ssim'))
        torch.cuda.synchronize()
    sys.exit(0)


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
    return statistics.median(ts[2:])


class Reads:
    """counts device-to-host reads while active"""
    names = ('cpu', 'item', 'tolist')

    def __enter__(self):
        self.n, self.orig = 0, {k: getattr(torch.Tensor, k) for k in self.names}
        for k, f in self.orig.items():
            def wrapped(t, *args, _f=f, **kw):
                self.n += bool(t.is_cuda)
                return _f(t, *args, **kw)
            setattr(torch.Tensor, k, wrapped)
        return self

    def __exit__(self, *exc):
        for k, f in self.orig.items():
            setattr(torch.Tensor, k, f)
        return False


def model_for(device_metrics):
    from textualdegremoval_amd.models import create_model
    kw = TI.HEADLINE
    cfg = O.default_cfg(**kw)
    net = dict(type='NAFNetRefFusion', enc_blk_nums=cfg['enc_blk_nums'], dec_blk_nums=cfg['dec_blk_nums'], middle_blk_num=cfg['middle_blk_num'],
               **{k: v for k, v in kw.items() if k not in ('enc_blk_nums', 'dec_blk_nums', 'middle_blk_num')})
    model = create_model({
        'model_type': 'RefGuidedImageCleanModel', 'num_gpu': 1, 'dist': False, 'is_train': True, 'network_g': net, 'path': {},
        'train': {'optim_g': {'type': 'AdamW', 'lr': 2e-4, 'ref_lr': 1e-4, 'weight_decay': 1e-4, 'betas': [0.9, 0.999]},
                  'scheduler': {'type': 'CosineAnnealingRestartCyclicLR', 'periods': [30, 70], 'restart_weights': [1, 1],
                                'eta_mins': [3e-4, 1e-6]},
                  'pixel_opt': {'type': 'L1Loss', 'loss_weight': 1, 'reduction': 'mean'},
                  'use_grad_clip': True, 'total_iter': 100, 'warmup_iter': -1},
        'logger': {'check_freq': 10 ** 9}, 'scale': 1,
        'val': {'session': True, 'device_metrics': device_metrics,
                'metrics': {'psnr': {'type': 'calculate_psnr', 'crop_border': 0, 'test_y_channel': False},
                            'ssim': {'type': 'calculate_ssim', 'crop_border': 0, 'test_y_channel': False}}}})
    model.net_g.load_state_dict(O.synth_params(cfg, seed=7), strict=True)
    return model


def validate(model, data):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.validation(data, 0, None, save_img=False, rgb2bgr=True, use_image=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, dict(model.metric_results)


res = dict(probe='val_metrics', device=torch.cuda.get_device_name(0), math=K.MATH, rounds=a.rounds, images=a.images,
           note='wall milliseconds of one validation of `images` images (forward replays included); synthetic weights, no quality claim',
           validation={}, kernels={})
models = {'a_host_loop': model_for(False), 'b_device_metrics': model_for(True)}
for H, W in SIZES:
    data = []
    for i in range(a.images):
        lq, gt, ref = O.synth_pair(1, H, W, seed=100 + i)
        data.append({'lq': lq, 'gt': gt, 'ref': ref})
    ts, reads, last = {k: [] for k in models}, {}, {}
    for k, m in models.items():
        for _ in range(2):
            validate(m, data)
        with Reads() as r:
            last[k] = validate(m, data)[1]
        reads[k] = r.n
    assert last['a_host_loop'] == last['b_device_metrics'], last
    for _ in range(a.rounds):
        for k, m in models.items():
            ts[k].append(validate(m, data)[0])
    ta, tb = ts['a_host_loop'], ts['b_device_metrics']
    res['validation'][f'{a.images}x3x{H}x{W}'] = dict(
        ms={k: stats(v) for k, v in ts.items()}, a_to_a_spread_ms=round(abs(statistics.median(ta[0::2]) - statistics.median(ta[1::2])), 3),
        ms_per_image_saved=round((statistics.median(ta) - statistics.median(tb)) / a.images, 3),
        device_to_host_reads_per_validation=reads, metric_results=last['b_device_metrics'], same_bits=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')
del models

for H, W in SIZES:
    p, g = (t.cuda() for t in pair(H, W, H))
    us = graph_us(lambda: K.val_metrics(p, g, what=('psnr', 'ssim')))
    hs = []
    for _ in range(a.rounds + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        x, y = M.tensor2img(p, rgb2bgr=True), M.tensor2img(g, rgb2bgr=True)
        M.calculate_psnr(x, y, 0), M.calculate_ssim(x, y, 0)
        hs.append((time.perf_counter() - t0) * 1e3)
    res['kernels'][f'1x3x{H}x{W}'] = dict(val_metrics_psnr_ssim_device_us=round(us, 1), host_path_wall_ms=stats(hs[2:]))
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
