"""InferenceSession.run_tiled(..., matcher=) measured, one process, one GPU, arithmetic bx3.  No pass bar: nobody has measured either form.
Headline network (NAFNetRefFusion width 32, enc [1, 1, 1, 28]), DINOv2 ViT-B/14 geometry with random weights (dino.random_vit_b14_state_dict:
the arithmetic does not depend on the values), tile 256, overlap 32, tile_batch 4.
  (a) lq and ref at 720 x 1280: 24 tiles, 8 x 17 = 136 windows.  The whole-ref form is refused there (MASA geometry) -- recorded.  Matched:
      the bank build alone (window_bank), one batch's match alone (match_bank), ms per image of the whole call (median of `--rounds` calls
      after eager / capture / replay), peak memory above what is resident, captures.
  (b) lq and ref at 768 x 768, where both forms run: matched against whole-ref tiled, the same medians and peaks.
Writes probe_tiled_match.json next to this file (or `--out PATH`).   python profiles/tiled_match/probe_tiled_match.py [--out PATH]"""
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
import torch  # noqa: E402

import test_hip_inference as TI  # noqa: E402
from textualdegremoval_amd import kernels as K  # noqa: E402
from textualdegremoval_amd.dino import DinoMatcher, random_vit_b14_state_dict  # noqa: E402
from textualdegremoval_amd.inference import InferenceSession  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(HERE, 'probe_tiled_match.json'))
ap.add_argument('--rounds', type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_tiled_match.py measures on the GPU'
K.set_math('bx3')
TILE = dict(tile=256, overlap=32, tile_batch=4)
res = dict(probe='tiled_match', device=torch.cuda.get_device_name(0), math=K.MATH, matcher='ViT-B/14, random weights, default arithmetic', **TILE)


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


def median_ms(fn, warm=2):
    for _ in range(warm):
        fn()
    return round(statistics.median(wall_ms(fn)[0] for _ in range(a.rounds)), 2)


def peak_and_ms(fn):
    for _ in range(3):                                                       # eager, capture + replay, replay
        out = fn()
    del out
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()                                     # (packs, graph pool, matcher weights are resident: not in the peak)
    torch.cuda.reset_peak_memory_stats()
    ms = [wall_ms(fn)[0] for _ in range(a.rounds)]
    return round(statistics.median(ms), 2), round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1), round(base / 2 ** 20, 1)


net = TI._guided_net(TI.HEADLINE, 7)
m = DinoMatcher(random_vit_b14_state_dict(seed=1), torch.device('cuda'))


def leg(lq, ref, matcher):
    sess = InferenceSession(net)
    try:
        ms, peak, resident = peak_and_ms(lambda: sess.run_tiled(lq, ref, matcher=matcher, **TILE))
        out = dict(median_ms_per_image=ms, peak_MiB_above_resident=peak, resident_MiB=resident, captures=sess.captures,
                   graphs_held=len(sess.graphs))
    except ValueError as e:
        out = dict(refused=f'{type(e).__name__}: {e}')
    sess.release()
    del sess
    gc.collect()
    torch.cuda.empty_cache()
    return out


def matcher_alone(lq, ref):
    bank = m.window_bank(ref, 256)
    tiles = torch.cat([lq[:, :, :256, 64 * i:64 * i + 256] for i in range(4)]).contiguous()
    rows = torch.zeros(4, dtype=torch.int32, device='cuda')
    out = dict(windows=bank.ny * bank.nx, grid=[bank.ny, bank.nx, bank.stride], bank_MiB=round(bank.feats.numel() * 4 / 2 ** 20, 1),
               bank_build_ms=median_ms(lambda: m.window_bank(ref, 256)),
               match_ms_per_batch=median_ms(lambda: m.match_bank(tiles, bank, rows, ref)))
    fl, T = m.tokens(K.resize_bilinear(tiles, 266, 266), flat=True)
    out['match_kernels_only_ms_per_batch'] = median_ms(lambda: K.token_match_bank(fl, bank.feats, rows, ref, 256, bank.stride, bank.nx, T + 1))
    return out


# ------------------------------------------------------------------ (a)
lq, ref = rand(1, 3, 720, 1280, seed=1), rand(1, 3, 720, 1280, seed=2)
res['a_720x1280'] = dict(tiles=24, whole_ref=leg(lq, ref, None), matched=leg(lq, ref, m), matcher_alone=matcher_alone(lq, ref))
write()
# ------------------------------------------------------------------ (b)
lq, ref = rand(1, 3, 768, 768, seed=3), rand(1, 3, 768, 768, seed=4)
res['b_768x768'] = dict(tiles=16, whole_ref=leg(lq, ref, None), matched=leg(lq, ref, m), matcher_alone=matcher_alone(lq, ref))
w, mt = res['b_768x768']['whole_ref'], res['b_768x768']['matched']
if 'median_ms_per_image' in w and 'median_ms_per_image' in mt:
    res['b_768x768']['matched_over_whole_ref'] = round(mt['median_ms_per_image'] / w['median_ms_per_image'], 2)
write()
print(json.dumps(res))
