"""inference.InferenceSession against the no-gradient forward it wraps, one process, one GPU, alternating a / b / a / b:
  (a) `with torch.no_grad(): net(...)` -- every weight packed afresh, every launch issued from the host (nafnet_arch_utils.infer_fwd);
  (b) `sess(...)` on a warm session -- weights packed once, the forward replayed as one hipGraph.
Per network: median / min device time of a forward (two events around one call), kernels per forward of both legs (torch.profiler; null
for (b) where the tracer reported nothing of the replayed graph in three tries),
pack kernels among those of (a), peak memory above the resident state (the session's own packs and graph pool are resident: recorded apart),
the number of packed weights.  The margin of the comparison is the
a-to-a spread of the same run (the medians of the even and of the odd rounds of (a)).
  headline NAFNetRefFusion width 32 enc [1, 1, 1, 28] at 1 x 3 x 512^2; NAFNetDynamicFusion width 32 at 1 x 3 x 256^2;
  RestormerRefFusion dim 48 [4, 6, 6, 8] at 1 x 3 x 256^2; the W8 NAFNetRefFusion of the tests at 2 x 3 x 256^2
and, at 1 x 3 x 512^2 on the headline network, bytes to bytes: `sess.run_u8` (upload uint8, one replay, download uint8) against the host
pipeline of the reference's evaluation loop (img2tensor on the host, upload float32, forward, download float32, tensor2img on the host);
wall-clock, synchronised.
Writes profiles/infer_session/probe_infer_session.json (or `--out PATH`).   python profiles/probe_infer_session.py [--out PATH] [--rounds R]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

import test_hip_dynfusion_inference as TD  # noqa: E402
import test_hip_inference as TI  # noqa: E402
import test_hip_restormer_inference as TR  # noqa: E402
from oracle import nafnet_ref_oracle as O  # noqa: E402
from textualdegremoval_amd import kernels as K  # noqa: E402
from textualdegremoval_amd.inference import InferenceSession  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'infer_session', 'probe_infer_session.json'))
ap.add_argument('--rounds', type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_infer_session.py measures on the GPU'
K.set_math('bx3')


def dev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    del out
    return (t1 - t0) * 1e3


def alternate(fa, fb, rounds, clock):
    for fn in (fa, fb, fa, fb):
        clock(fn)
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(clock(fa))
        tb.append(clock(fb))
    return ta, tb


def peak(fn):
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    p = torch.cuda.max_memory_allocated() - base
    del out
    return p


def kernels_of(fn):
    """(device kernels of one call, those whose name says pack_weights)"""
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    del out
    names = [ev.name for ev in prof.events() if ev.device_type is not None and str(ev.device_type).endswith('CUDA')
             and 'Memcpy' not in ev.name and 'Memset' not in ev.name]
    return len(names), sum(1 for n in names if 'pack_weights' in n)


def stats(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


def compare(ta, tb):
    """b against a with the a-to-a spread of the run as the margin"""
    spread = abs(statistics.median(ta[0::2]) - statistics.median(ta[1::2]))
    ma, mb = statistics.median(ta), statistics.median(tb)
    return dict(a_to_a_spread_ms=round(spread, 3), b_minus_a_ms=round(mb - ma, 3), speedup=round(ma / mb, 3),
                b_not_slower=bool(mb <= ma + spread))


def write(res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


def headline():
    net = TI._guided_net(TI.HEADLINE, 7)
    lq, _, ref = O.synth_pair(1, 512, 512, seed=77)
    return net, (lq.cuda(), ref.cuda())


def dynfusion():
    net, _ = TD._wide_net([1, 1, 1, 28], 3)
    gen = torch.Generator().manual_seed(9)
    return net, (torch.rand(1, 3, 256, 256, generator=gen).cuda(), torch.randn(1, 10, 1024, generator=gen).cuda())


def restormer():
    net, lq, ref = TR._cfg3()
    return net, (lq, ref)


def w8():
    net = TI._guided_net(TI.W8, 3)
    lq, _, ref = O.synth_pair(2, 256, 256, seed=1237)
    return net, (lq.cuda(), ref.cuda())


res = dict(probe='infer_session', device=torch.cuda.get_device_name(0), math=K.MATH, rounds=a.rounds, networks={})
for name, make in (('NAFNetRefFusion_w32_512', headline), ('NAFNetDynamicFusion_w32_256', dynfusion), ('RestormerRefFusion_d48_256', restormer),
                   ('NAFNetRefFusion_w8_b2_256', w8)):
    net, images = make()
    torch.cuda.synchronize()
    resident0 = torch.cuda.memory_allocated()
    sess = InferenceSession(net)

    def fa():
        with torch.no_grad():
            return net(*images)

    def fb():
        return sess(*images)
    want = fa()
    same = all(torch.equal(fb(), want) for _ in range(3))                   # eager, capture + replay, replay
    gc.collect()
    torch.cuda.synchronize()
    resident = torch.cuda.memory_allocated() - resident0 - want.numel() * 4     # packs + the graph's pool (static inputs, output, intermediates)
    ta, tb = alternate(fa, fb, a.rounds, dev_ms)
    ka, kb = kernels_of(fa), kernels_of(fb)
    for _ in range(3):                                                       # (the tracer sometimes reports nothing of a replayed graph)
        if kb[0]:
            break
        kb = kernels_of(fb)
    seen = kb[0] > 0
    n_packed = len(sess.plan.entries)
    ent = dict(shape=[list(t.shape) for t in images], bit_identical=bool(same), packed_weights=n_packed,
               forward_ms=dict(a_no_grad=stats(ta), b_session=stats(tb)), **compare(ta, tb),
               kernels_per_forward=dict(a_no_grad=ka[0], a_pack_kernels=ka[1], b_session=kb[0] if seen else None,
                                        b_pack_kernels=kb[1] if seen else None, b_seen_by_the_tracer=seen),
               kernels_fewer_by_at_least_the_packs=bool(kb[0] <= ka[0] - n_packed) if seen else None,
               peak_memory_MiB=dict(a_no_grad=round(peak(fa) / 2 ** 20, 1), b_session=round(peak(fb) / 2 ** 20, 1)),
               session_resident_MiB=round(resident / 2 ** 20, 1))
    res['networks'][name] = ent
    write(res)
    if name == 'NAFNetRefFusion_w32_512':
        # ---- bytes to bytes at 1 x 3 x 512 x 512
        rng = np.random.default_rng(5)
        lq8, ref8 = (rng.integers(0, 256, size=(512, 512, 3), dtype=np.uint8) for _ in range(2))

        def host():
            def to_t(img):                                                   # imfrombytes(float32=True) + img2tensor(bgr2rgb=True)
                x = img.astype(np.float32) / 255.
                return torch.from_numpy(np.ascontiguousarray(x[..., ::-1].transpose(2, 0, 1))).float().unsqueeze(0).cuda()
            with torch.no_grad():
                out = net(to_t(lq8), to_t(ref8))
            t = out.squeeze(0).float().detach().cpu().clamp_(0, 1)            # tensor2img(rgb2bgr=True)
            img = np.ascontiguousarray(t.numpy().transpose(1, 2, 0)[..., ::-1])
            return (img * 255.0).round().astype(np.uint8)

        def dev():
            lq, ref = torch.from_numpy(lq8).unsqueeze(0).cuda(), torch.from_numpy(ref8).unsqueeze(0).cuda()
            return sess.run_u8(lq, ref, bgr=True).cpu().numpy()[0]
        same8 = all(np.array_equal(dev(), host()) for _ in range(3))
        th, td = alternate(host, dev, a.rounds, wall_ms)
        res['bytes_to_bytes_512'] = dict(bit_identical=bool(same8), wall_ms=dict(a_host_pipeline=stats(th), b_run_u8=stats(td)), **compare(th, td))
        write(res)
    sess.release()
    del sess, net, images, want
    gc.collect()
    torch.cuda.empty_cache()
res['acceptance'] = dict(replay_not_slower_everywhere=all(v['b_not_slower'] for v in res['networks'].values()),
                         kernels_fewer_wherever_the_tracer_saw_the_graph=all(v['kernels_fewer_by_at_least_the_packs'] is not False
                                                                            for v in res['networks'].values()))
write(res)
print(json.dumps(res))
