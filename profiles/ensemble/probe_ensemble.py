"""The self-ensemble's two kernels (csrc/tdr_dihedral.hip) and InferenceSession.run_ensemble, one process, one GPU, bx3.  No pass bar.
  kernels, at 1 x 3 x 512^2 and 1 x 3 x 720 x 1280: tdr_dihedral_gather per op (float source) and tdr_dihedral_mean over all 8 members
    (float and byte output).  Time: REPS launches captured into one hipGraph, two events around a replay, over REPS -- the device time of
    a launch including the gap to the next one, without the host's launch cost; median of `--rounds` replays.  Bytes: read plus write of
    the tensors of the entry point (gather: source + one output; mean: 8 members + the output).  The tensors are far smaller than the
    256 MiB Infinity Cache and are re-used by every launch: the GB/s are cache-resident rates, to be compared with op 0 (the plain
    copy of the same kernel at the same size), not with the HBM peak.  Each op is reported as a ratio to op 0.
  network, the headline NAFNetRefFusion (width 32, enc [1, 1, 1, 28]) at 1 x 3 x 512^2 with a 512^2 ref: a warm
    sess.run_ensemble(lq, ref, ops=8) (two gathers per class, ONE forward of 4 images per class, one mean) against eight separate warm
    sess(...) calls around torch.flip / transpose(...).contiguous(), seven ATen adds and a division; alternating, device events,
    medians; captures and peak memory above the resident state of both.  The two are not the same computation bit for bit (a stack of
    4 against single images): the largest difference is recorded.
No restoration-quality figure: there are no trained weights here, the networks carry synthetic ones -- nothing below says anything about
what the ensemble gains in PSNR.
Writes profiles/ensemble/probe_ensemble.json (or `--out PATH`).   python profiles/ensemble/probe_ensemble.py [--out PATH] [--rounds R]"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402

import test_hip_inference as TI  # noqa: E402
from oracle import nafnet_ref_oracle as O  # noqa: E402
from textualdegremoval_amd import kernels as K  # noqa: E402
from textualdegremoval_amd.inference import InferenceSession, dihedral, dihedral_inverse  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ensemble', 'probe_ensemble.json'))
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--reps', type=int, default=20)
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_ensemble.py measures on the GPU'
K.set_math('bx3')


def write(res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


def graph_us(fn):
    """median device microseconds of one fn(): a.reps of them in a captured graph, events around each of a.rounds replays"""
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


def rate(us, nbytes):
    return dict(us=round(us, 2), GBps=round(nbytes / us * 1e-3, 1))


res = dict(probe='ensemble', device=torch.cuda.get_device_name(0), math=K.MATH, rounds=a.rounds, launches_per_graph=a.reps,
           note='kernel GB/s are cache-resident rates (tensors of 3 - 90 MB, re-used by every launch); compare with op 0, not with the HBM peak. '
                'No restoration-quality claim: synthetic weights.', kernels={})
for N, C, H, W in ((1, 3, 512, 512), (1, 3, 720, 1280)):
    gen = torch.Generator().manual_seed(H)
    x = torch.rand(N, C, H, W, generator=gen).cuda()
    plane_bytes = N * C * H * W * 4
    ent = dict(gather_f32={}, mean={})
    for op in range(8):
        assert torch.equal(K.dihedral_gather(x, (op,)), dihedral(x, op).contiguous())
        ent['gather_f32'][f'op{op}'] = rate(graph_us(lambda: K.dihedral_gather(x, (op,))), 2 * plane_bytes)
    for op in range(1, 8):
        ent['gather_f32'][f'op{op}']['rate_vs_op0'] = round(ent['gather_f32']['op0']['us'] / ent['gather_f32'][f'op{op}']['us'], 3)
    for name, sel in (('straight_0123', (0, 1, 2, 3)), ('transposed_4567', (4, 5, 6, 7))):
        ent['gather_f32'][name] = rate(graph_us(lambda: K.dihedral_gather(x, sel)), 5 * plane_bytes)
    straight, transposed = K.dihedral_gather(x, (0, 1, 2, 3)), K.dihedral_gather(x, (4, 5, 6, 7))
    for op in (0, 7):                                                                         # (one member: its inverse, divided by 1.0f)
        assert torch.equal(K.dihedral_mean(*((straight[:N], None) if op < 4 else (None, transposed[3 * N:])), (op,), N), x)
    ent['mean']['all8_f32'] = rate(graph_us(lambda: K.dihedral_mean(straight, transposed, tuple(range(8)), N)), 9 * plane_bytes)
    ent['mean']['all8_u8'] = rate(graph_us(lambda: K.dihedral_mean(straight, transposed, tuple(range(8)), N, u8=True)),
                                  8 * plane_bytes + N * C * H * W)
    ent['mean']['straight4_f32'] = rate(graph_us(lambda: K.dihedral_mean(straight, None, (0, 1, 2, 3), N)), 5 * plane_bytes)
    ent['mean']['transposed4_f32'] = rate(graph_us(lambda: K.dihedral_mean(None, transposed, (4, 5, 6, 7), N)), 5 * plane_bytes)
    ent['mean']['transposed4_vs_straight4'] = round(ent['mean']['straight4_f32']['us'] / ent['mean']['transposed4_f32']['us'], 3)
    # op 0 as the yardstick of the mean: one member, a plain copy divided by 1.0f; and the ATen chain the kernels replace
    ent['mean']['op0_f32'] = rate(graph_us(lambda: K.dihedral_mean(x, None, (0,), N)), 2 * plane_bytes)
    ent['aten_flip_transpose_contiguous_op7'] = rate(graph_us(lambda: dihedral(x, 7).contiguous()), 2 * plane_bytes)
    res['kernels'][f'{N}x{C}x{H}x{W}'] = ent
    write(res)
    del x, straight, transposed


def dev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


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


def stats(ts):
    return dict(median=round(statistics.median(ts), 3), min=round(min(ts), 3), max=round(max(ts), 3))


net = TI._guided_net(TI.HEADLINE, 7)
lq, _, ref = O.synth_pair(1, 512, 512, seed=77)
lq, ref = lq.cuda(), ref.cuda()
sess_a, sess_b = InferenceSession(net), InferenceSession(net)


def separate():
    s = None
    for op in range(8):
        v = dihedral_inverse(sess_a(dihedral(lq, op).contiguous(), dihedral(ref, op).contiguous()), op)
        s = v.contiguous() if s is None else s + v
    return s / 8


def ensemble():
    return sess_b.run_ensemble(lq, ref, ops=8)


for fn in (separate, ensemble, separate, ensemble, separate, ensemble):              # eager, capture + replay, replay
    want = fn()
diff = (separate() - ensemble()).abs().max().item()
ta, tb = [], []
for _ in range(a.rounds):
    ta.append(dev_ms(separate))
    tb.append(dev_ms(ensemble))
spread = abs(statistics.median(ta[0::2]) - statistics.median(ta[1::2]))
res['network'] = dict(name='NAFNetRefFusion_w32_512', lq=list(lq.shape), ref=list(ref.shape),
                      ms=dict(a_eight_separate_calls=stats(ta), b_run_ensemble=stats(tb)), a_to_a_spread_ms=round(spread, 3),
                      speedup=round(statistics.median(ta) / statistics.median(tb), 3),
                      captures=dict(a_eight_separate_calls=sess_a.captures, b_run_ensemble=sess_b.captures),
                      graphs=dict(a_eight_separate_calls=len(sess_a.graphs), b_run_ensemble=len(sess_b.graphs)),
                      peak_memory_MiB=dict(a_eight_separate_calls=round(peak(separate) / 2 ** 20, 1), b_run_ensemble=round(peak(ensemble) / 2 ** 20, 1)),
                      max_abs_difference_a_b=diff, output_abs_max=want.abs().max().item())
write(res)
print(json.dumps(res))
