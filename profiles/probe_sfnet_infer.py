"""SFNet's forward-only route against the eval pass on the training walk, one process, one GPU, legs alternating a ... f per round:
  (a) sfnet_engine.net_fwd(training=False, keep=True)   -- the eval pass before this route existed: every `saved` tuple built, per-op kernels;
  (b) keep=False with sfnet_engine.INFER_KERNELS = False -- nothing saved, GELU in place, gelu_ + region_affine_fwd per op;
  (c) keep=False, fused                                   -- GELU -> Gap / Patch_ap on tdr_sf_act_region_sums / _apply;
  (d) a warm inference.InferenceSession                   -- weights packed once, (c) replayed as one hipGraph;
  (e) a session with max_graphs=0                         -- weights packed once, (c) launched from the host on every call;
  (f) `with torch.no_grad(): net(x)`                      -- what a session call replaces: (c) behind the module's own host work;
  (g) the engine call of (c) under a resident pack plan   -- (e) without the module's host work: what the resident packs alone change.
Legs (a)-(c) are engine calls on a prebuilt parameter dict; (d)-(f) start at the module, whose per-call host work (walking the module tree
for parameters and buffers: infer_spec(), the session's staleness check) falls between the two events as well -- recorded apart as `host_ms`.
SFNet(['train', 'Indoor'], num_res=16) after .eval(), bx3, 1 x 3 x 256 x 256.  Per leg: median / min device time of a forward (two
events around one call), kernels per forward, pack kernels among them and the sum of the kernels' own durations (torch.profiler; the
tracer's record of a replayed graph is incomplete: null where it reported nothing), peak memory above the resident state.  The margin of
every comparison is the a-to-a spread of the same run (the medians of the even and of the odd rounds of (a)).
One ordinary ResBlock per level -- (N, C, H, W) = (1, 32, 256, 256), (1, 64, 128, 128), (1, 128, 64, 64) -- on the per-op and on the fused
path: the whole block (conv1 .. conv2) and the part between the convolutions alone, `--reps` back-to-back calls between two events.
Writes profiles/sfnet_infer/probe_sfnet_infer.json (or `--out PATH`).   python profiles/probe_sfnet_infer.py [--out PATH] [--rounds R]"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from oracle import sfnet_oracle as SO  # noqa: E402
from textualdegremoval_amd import kernels as K  # noqa: E402
from textualdegremoval_amd import sfnet_engine as SE  # noqa: E402
from textualdegremoval_amd.inference import InferenceSession  # noqa: E402
from textualdegremoval_amd.models.archs import define_network  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sfnet_infer', 'probe_sfnet_infer.json'))
ap.add_argument('--rounds', type=int, default=20)
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--num-res', type=int, default=16)
ap.add_argument('--size', type=int, default=256)
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_sfnet_infer.py measures on the GPU'
K.set_math('bx3')


def dev_ms(fn, reps=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1) / reps


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
    """(device kernels of one call, those whose name says pack_weights, the sum of the kernels' durations in ms)"""
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    del out
    evs = [ev for ev in prof.events() if ev.device_type is not None and str(ev.device_type).endswith('CUDA')
           and 'Memcpy' not in ev.name and 'Memset' not in ev.name]
    busy = sum(ev.time_range.elapsed_us() for ev in evs) / 1e3            # (the device-side interval of each kernel event)
    by = {}
    for ev in evs:
        n = ev.name.replace('void ', '').replace('(anonymous namespace)::', '').split('(')[0][:70]
        c, t = by.get(n, (0, 0.0))
        by[n] = (c + 1, t + ev.time_range.elapsed_us())
    top = sorted(by.items(), key=lambda kv: -kv[1][1])[:14]
    return len(evs), sum(1 for ev in evs if 'pack_weights' in ev.name), busy, {n: dict(launches=c, total_us=round(t, 1)) for n, (c, t) in top}


def stats(ts):
    return dict(median=round(statistics.median(ts), 4), min=round(min(ts), 4), max=round(max(ts), 4))


def spread_of(ta):
    return abs(statistics.median(ta[0::2]) - statistics.median(ta[1::2]))


def compare(tx, ty, spread):
    """y against x: not slower by more than the a-to-a spread of the run"""
    mx, my = statistics.median(tx), statistics.median(ty)
    return dict(y_minus_x_ms=round(my - mx, 4), speedup=round(mx / my, 3), y_not_slower=bool(my <= mx + spread))


def write(res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


class fused:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev, SE.INFER_KERNELS = SE.INFER_KERNELS, self.on

    def __exit__(self, *exc):
        SE.INFER_KERNELS = self.prev
        return False


res = dict(probe='sfnet_infer', device=torch.cuda.get_device_name(0), math=K.MATH, rounds=a.rounds, num_res=a.num_res,
           shape=[1, 3, a.size, a.size])
net = define_network(dict(type='SFNet', mode=['train', 'Indoor'], num_res=a.num_res)).cuda()
sd = SO.synth_state(a.num_res, seed=41)
for k in sd:                                            # (as tests/test_hip_sfnet.py at this depth: residual branches small, activations O(1))
    if k.endswith('conv2.main.0.weight'):
        sd[k] = sd[k] * 0.2
net.load_state_dict(sd)
net.eval()
x = torch.rand(1, 3, a.size, a.size, generator=torch.Generator().manual_seed(42)).cuda()
P = {k: v.detach() for k, v in list(net.named_parameters()) + list(net.named_buffers())}
torch.cuda.synchronize()
resident0 = torch.cuda.memory_allocated()
sess = InferenceSession(net)
sess0 = InferenceSession(net, max_graphs=0)


def fa():
    return SE.net_fwd(P, x, a.num_res, training=False, keep=True)[0]


def fb():
    with fused(False):
        return SE.net_fwd(P, x, a.num_res, training=False, keep=False)[0]


def fc():
    with fused(True):
        return SE.net_fwd(P, x, a.num_res, training=False, keep=False)[0]


def fd():
    return sess(x)


def fe():
    return sess0(x)


def ff():
    with torch.no_grad():
        return net(x)


def host_ms(fn, n=20):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 4)


plan_g = K.PackPlan(admit=[t.data_ptr() for t in P.values()])
plan_g.valid = True


def fg():
    prev = K.set_pack_plan(plan_g)
    try:
        return fc()
    finally:
        K.set_pack_plan(prev)


legs = (('a_keep', fa), ('b_perop', fb), ('c_fused', fc), ('d_session', fd), ('e_session_packs_only', fe), ('f_module', ff),
        ('g_engine_resident_packs', fg))
want_a, want_c = fa(), fc()
res['bit_identical'] = dict(b_to_a=all(torch.equal(p, q) for p, q in zip(fb(), want_a)),
                            d_to_c=all(all(torch.equal(p, q) for p, q in zip(fd(), want_c)) for _ in range(3)))     # eager, capture + replay, replay
res['max_abs_c_minus_a'] = max((p - q).abs().max().item() for p, q in zip(want_c, want_a))
gc.collect()
torch.cuda.synchronize()
res['session_resident_MiB'] = round((torch.cuda.memory_allocated() - resident0 - 2 * sum(t.numel() * 4 for t in want_a)) / 2 ** 20, 1)
res['packed_weights'] = len(sess.plan.entries)
for _ in range(2):
    for _, fn in legs:
        dev_ms(fn)
ts = {name: [] for name, _ in legs}
for _ in range(a.rounds):
    for name, fn in legs:
        ts[name].append(dev_ms(fn))
spread = spread_of(ts['a_keep'])
res['forward_ms'] = {name: stats(t) for name, t in ts.items()}
res['a_to_a_spread_ms'] = round(spread, 4)
res['comparisons'] = dict(b_against_a=compare(ts['a_keep'], ts['b_perop'], spread), c_against_b=compare(ts['b_perop'], ts['c_fused'], spread),
                          d_against_c=compare(ts['c_fused'], ts['d_session'], spread),
                          e_against_c=compare(ts['c_fused'], ts['e_session_packs_only'], spread),
                          d_against_e=compare(ts['e_session_packs_only'], ts['d_session'], spread),
                          d_against_f=compare(ts['f_module'], ts['d_session'], spread),
                          g_against_c=compare(ts['c_fused'], ts['g_engine_resident_packs'], spread),
                          d_against_g=compare(ts['g_engine_resident_packs'], ts['d_session'], spread))
res['host_ms'] = dict(session_staleness_check=host_ms(sess.stale), infer_spec=host_ms(net.infer_spec))
write(res)
kern = {}
for name, fn in legs:
    kk = kernels_of(fn)
    for _ in range(3):                                  # (the tracer sometimes reports nothing of a replayed graph)
        if kk[0]:
            break
        kk = kernels_of(fn)
    kern[name] = dict(kernels=kk[0] or None, pack_kernels=kk[1] if kk[0] else None, sum_of_kernel_durations_ms=round(kk[2], 3) if kk[0] else None)
    if name in ('c_fused', 'e_session_packs_only', 'g_engine_resident_packs', 'd_session'):
        kern[name]['by_kernel'] = kk[3]
res['kernels_per_forward'] = kern
res['peak_memory_MiB'] = {name: round(peak(fn) / 2 ** 20, 1) for name, fn in legs}
write(res)

# ---- one ordinary ResBlock per level, per-op against fused
blocks = {}
for lvl, (C, S) in enumerate(((32, a.size), (64, a.size // 2), (128, a.size // 4))):
    pre = f'Encoder.{lvl}.layers.0.'
    h = C // 2
    xb = torch.randn(1, C, S, S, generator=torch.Generator().manual_seed(50 + lvl)).cuda()
    gap = (P[pre + 'global_ap.fscale_h'], P[pre + 'global_ap.fscale_d'])
    pap = (P[pre + 'localap.h'], P[pre + 'localap.l'])
    zb, rb = torch.empty_like(xb), torch.empty_like(xb)

    def mid_perop():
        zb.copy_(xb)                                    # (the GELU is in place: start from the same pre-activation every time)
        K.gelu_(zb)
        K.region_affine_fwd(zb[:, :h], *gap, 1.0, 1, rb[:, :h])
        K.region_affine_fwd(zb[:, h:], *pap, 0.0, 2, rb[:, h:])
        return rb

    def mid_fused():
        zb.copy_(xb)
        return K.sf_act_region_affine(zb, *gap, *pap, 1, out=zb)

    def blk_perop():
        return SE.infer_res(xb, P, pre, False, SE.InferMode(None, False))

    def blk_fused():
        return SE.infer_res(xb, P, pre, False, SE.InferMode(None, True))

    def copy_only():
        zb.copy_(xb)
        return zb
    pairs = dict(between_convs=(mid_perop, mid_fused), whole_block=(blk_perop, blk_fused))
    ent = dict(shape=[1, C, S, S], chunks=list(K.sf_region_chunks(S, S)))
    tc = [dev_ms(copy_only, a.reps) for _ in range(a.rounds)]
    ent['copy_in_ms'] = stats(tc)                       # what both `between_convs` figures contain
    for what, (f0, f1) in pairs.items():
        for fn in (f0, f1, f0, f1):
            dev_ms(fn, a.reps)
        t0, t1 = [], []
        for _ in range(a.rounds):
            t0.append(dev_ms(f0, a.reps))
            t1.append(dev_ms(f1, a.reps))
        sp = spread_of(t0)
        ent[what] = dict(perop_ms=stats(t0), fused_ms=stats(t1), perop_to_perop_spread_ms=round(sp, 4), **compare(t0, t1, sp))
    blocks[f'level{lvl + 1}'] = ent
res['ordinary_resblock'] = blocks
res['acceptance'] = dict(c_not_slower_than_b=res['comparisons']['c_against_b']['y_not_slower'],
                         d_not_slower_than_c=res['comparisons']['d_against_c']['y_not_slower'],
                         d_not_slower_than_the_module_forward=res['comparisons']['d_against_f']['y_not_slower'],
                         fused_not_slower_at_every_level=all(v['between_convs']['y_not_slower'] and v['whole_block']['y_not_slower']
                                                             for v in blocks.values()))
write(res)
sess.release()
sess0.release()

# ---- does a TLSC network (mode[0] == 'test') capture?  Tried last, not required: the answer is recorded, nothing depends on it
tnet = define_network(dict(type='SFNet', mode=['test', 'Outdoor'], num_res=1)).cuda()
tnet.load_state_dict(SO.synth_state(1, seed=7))
tnet.eval()
tx = torch.rand(1, 3, 32, 48, generator=torch.Generator().manual_seed(11)).cuda()
twant = tnet(tx)
tsess = InferenceSession(tnet, max_graphs=1)
try:
    same = all(all(torch.equal(p, q) for p, q in zip(tsess(tx), twant)) for _ in range(3))
    res['tlsc_capture'] = dict(works=bool(tsess.captures == 1 and tsess.replays == 2), bit_identical=bool(same))
except NotImplementedError as e:
    res['tlsc_capture'] = dict(works=False, error=str(e)[:300])
write(res)
tsess.release()
print(json.dumps(res))
