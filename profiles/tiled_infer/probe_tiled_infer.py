"""InferenceSession.run_tiled measured, one process, one GPU, arithmetic bx3.  No pass bar: nobody has measured any of this before.
  (a) a validation folder emulated by eight images of eight sizes between 256^2 and 720 x 1280 on the headline network (NAFNetRefFusion
      width 32, enc [1, 1, 1, 28]), two passes each way: `sess(x, ref)` per shape with max_graphs=4 against `run_tiled(x, ref, tile=256)`.
      Captures, eager forwards and the median wall-clock ms per image of each pass.  The MASA geometry wants lq and ref of one aspect, so
      the full-frame leg takes a ref of the image's size and the tiled leg a 256^2 ref (the tile's): the legs time what each would run in
      practice, their outputs are not compared.
  (b) tiled against full-frame `sess(x)` on an un-guided NAFNet (width 32, enc [1, 1, 1, 28], random weights) at 1 x 3 x 512^2 and
      1 x 3 x 720 x 1280: ms per image, peak memory, and how far the per-tile statistics move the result (max |diff|, PSNR of one output
      against the other) -- informational.
  (c) the two kernels of csrc/tdr_tile.hip alone at 1 x 3 x 720 x 1280, tile 256, overlap 32: us per launch (device events around a
      train of back-to-back launches, so launch overhead is in it) and achieved GB/s from the bytes each must move; tdr_img_u8_to_planes on
      the same image beside them as the streaming yardstick.
Writes probe_tiled_infer.json next to this file (or `--out PATH`).   python profiles/tiled_infer/probe_tiled_infer.py [--out PATH]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import test_hip_inference as TI  # noqa: E402
from textualdegremoval_amd import kernels as K  # noqa: E402
from textualdegremoval_amd.inference import InferenceSession, TilePlan  # noqa: E402
from textualdegremoval_amd.models.archs import define_network  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'probe_tiled_infer.json'))
ap.add_argument('--rounds', type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_tiled_infer.py measures on the GPU'
K.set_math('bx3')
SIZES = [(256, 256), (320, 480), (384, 384), (480, 640), (512, 512), (540, 960), (600, 800), (720, 1280)]
res = dict(probe='tiled_infer', device=torch.cuda.get_device_name(0), math=K.MATH, tile=256, overlap=32, tile_batch=4)


def write():
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    return (t1 - t0) * 1e3, out


def rand(*shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed)).cuda()


def count_forwards(sess):
    """every Python forward of the session (eager ones and the one a capture runs)"""
    n, orig = [0], sess._forward

    def fwd(images):
        n[0] += 1
        return orig(images)
    sess._forward = fwd
    return n


# ------------------------------------------------------------------ (a)
net = TI._guided_net(TI.HEADLINE, 7)
images = [rand(1, 3, H, W, seed=100 + i) for i, (H, W) in enumerate(SIZES)]
refs_full = [rand(1, 3, H, W, seed=200 + i) for i, (H, W) in enumerate(SIZES)]
ref_tile = rand(1, 3, 256, 256, seed=300)
legs = {}
for leg in ('per_shape_session', 'run_tiled'):
    sess = InferenceSession(net, max_graphs=4)
    forwards = count_forwards(sess)
    passes = []
    for p in range(2):
        c0, r0, f0 = sess.captures, sess.replays, forwards[0]
        ms = []
        for x, rf in zip(images, refs_full):
            t, _ = wall_ms((lambda: sess(x, rf)) if leg == 'per_shape_session' else (lambda: sess.run_tiled(x, ref_tile, tile=256, overlap=32, tile_batch=4)))
            ms.append(round(t, 2))
        caps = sess.captures - c0
        passes.append(dict(captures=caps, replays=sess.replays - r0, eager_forwards=forwards[0] - f0 - caps,
                           ms_per_image=ms, median_ms_per_image=round(statistics.median(ms), 2), total_ms=round(sum(ms), 1)))
    legs[leg] = dict(passes=passes, graphs_held=len(sess.graphs))
    sess.release()
    del sess
    gc.collect()
    torch.cuda.empty_cache()
res['a_validation_folder'] = dict(network='NAFNetRefFusion w32 enc [1,1,1,28]', sizes=SIZES, **legs,
                                  tiled_faster_on_pass_2=bool(legs['run_tiled']['passes'][1]['total_ms'] < legs['per_shape_session']['passes'][1]['total_ms']))
write()
del net, images, refs_full
gc.collect()
torch.cuda.empty_cache()

# ------------------------------------------------------------------ (b)
torch.manual_seed(11)
net = define_network(dict(type='NAFNet', img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1])).cuda()


def peak_and_ms(fn):
    for _ in range(3):                                                       # eager, capture + replay, replay
        out = fn()
    del out
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()                                     # (the session's packs and graph pool are resident: not in the peak)
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(a.rounds):
        t, out = wall_ms(fn)
        ms.append(t)
    return out, round(statistics.median(ms), 2), round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1), round(base / 2 ** 20, 1)


res['b_tiled_against_full_frame'] = {}
for H, W in ((512, 512), (720, 1280)):
    x = rand(1, 3, H, W, seed=400 + H)
    ent = {}
    outs = {}
    for leg in ('full_frame', 'run_tiled'):
        sess = InferenceSession(net)
        outs[leg], ms, peak, resident = peak_and_ms((lambda: sess(x)) if leg == 'full_frame' else (lambda: sess.run_tiled(x, tile=256, overlap=32, tile_batch=4)))
        ent[leg] = dict(median_ms=ms, peak_MiB_above_resident=peak, resident_MiB=resident)
        sess.release()
        del sess
        gc.collect()
        torch.cuda.empty_cache()
    d = (outs['run_tiled'].double() - outs['full_frame'].double())
    ent['max_abs_diff'] = float(d.abs().max())
    ent['psnr_dB_of_one_against_the_other'] = round(float(-10 * torch.log10((d * d).mean())), 2)
    res['b_tiled_against_full_frame'][f'{H}x{W}'] = ent
    write()
del net, outs
gc.collect()
torch.cuda.empty_cache()

# ------------------------------------------------------------------ (c)
H, W, LAUNCHES = 720, 1280, 200
plan = TilePlan(1, H, W, (256, 256), 32, 4, 'cuda')
T = plan.n_tiles
x = rand(1, 3, H, W, seed=500)
u8 = torch.from_numpy(np.random.default_rng(6).integers(0, 256, size=(1, H, W, 3), dtype=np.uint8)).cuda()
tiles = K.tile_gather(x, plan.table[:T], plan.th, plan.tw)
tile_bytes, img_bytes = T * 3 * plan.th * plan.tw * 4, 3 * H * W * 4


def train_us(fn):
    for _ in range(20):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = []
    for _ in range(5):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(LAUNCHES):
            fn()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / LAUNCHES)
    return statistics.median(best)


kern = {}
for name, fn, nbytes in (('tile_gather_f32', lambda: K.tile_gather(x, plan.table[:T], plan.th, plan.tw), 2 * tile_bytes),
                         ('tile_gather_u8', lambda: K.tile_gather(u8, plan.table[:T], plan.th, plan.tw), tile_bytes // 4 + tile_bytes),
                         ('tile_blend', lambda: K.tile_blend(tiles, 1, H, W, plan.ytabs, plan.xtabs), tile_bytes + img_bytes),
                         ('img_u8_to_planes', lambda: K.img_u8_to_planes(u8), img_bytes // 4 + img_bytes)):
    us = train_us(fn)
    kern[name] = dict(us_per_launch=round(us, 2), bytes=nbytes, GB_per_s=round(nbytes / us / 1e3, 1))
res['c_kernels_alone'] = dict(shape=[1, 3, H, W], tiles=T, launches_per_train=LAUNCHES,
                              note='back-to-back launches through the Python wrappers, output allocation included', **kern)
write()
print(json.dumps(res))
