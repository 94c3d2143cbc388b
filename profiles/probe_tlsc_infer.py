"""The TLSC block on the fused forward-only chains (engine.naf_fwd_local with engine.LOCAL_KERNELS: tdr_naf_head_infer, depthwise + gate,
box mean, tdr_naf_tail_infer_local) against the per-op launches it replaces (LOCAL_KERNELS = False), one process, alternating runs:
  * one block per chain level -- c = 32 at 512^2, 64 at 256^2, 128 at 128^2, 256 at 64^2, each under the box `train_size=(1, 3, 256, 256)`
    gives at that level: device time per block in us (two events around 8 blocks, weight packs cached in a PackPlan);
  * the whole `NAFNetLocal`, width 32, enc [1, 1, 1, 28], at 1 x 3 x 720 x 1280: device time of a forward, peak memory above the resident
    state, device kernels per forward (torch.profiler: every kernel of the process, the library's included);
  * the error figures of tests/test_hip_tlsc_fused.py::test_fused_block_against_float64 (its cases, its float64 restatement).
Writes profiles/tlsc_infer/probe_tlsc_infer.json (or `--out PATH`) and prints it.   python profiles/probe_tlsc_infer.py [--out PATH] [--rounds R]"""
import argparse
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

import test_hip_tlsc_fused as T  # noqa: E402  (the block cases, their inputs and the float64 restatement)
from textualdegremoval_amd import engine as E, kernels as K  # noqa: E402
from textualdegremoval_amd.models.archs import define_network  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tlsc_infer', 'probe_tlsc_infer.json'))
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--hw', type=int, nargs=2, default=[720, 1280])
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_tlsc_infer.py measures on the GPU'
K.set_math('bx3')
REP = 8


def switched(on, fn):
    def run():
        prev, E.LOCAL_KERNELS = E.LOCAL_KERNELS, on
        try:
            return fn()
        finally:
            E.LOCAL_KERNELS = prev
    return run


def dev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    del out
    return e0.elapsed_time(e1)


def alternate(fns, rounds):
    """{name: [ms per round]}: every round runs each variant once, in turn (same clocks, same neighbours on the host)"""
    for fn in fns.values():
        dev_ms(fn)
        dev_ms(fn)
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(dev_ms(fn))
    return ts


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
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    del out
    return sum(1 for ev in prof.events() if ev.device_type is not None and str(ev.device_type).endswith('CUDA')
               and 'Memcpy' not in ev.name and 'Memset' not in ev.name)


def write(res):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


res = dict(probe='tlsc_infer', device=torch.cuda.get_device_name(0), math=K.MATH, rounds=a.rounds)

# ---- one block per level
cfg4 = dict(enc_blk_nums=[1, 1, 1, 1])
boxes = E.tlsc_kernel_sizes(cfg4, (1, 3, 256, 256))
blocks = []
plan = K.PackPlan()
for level, (c, hw) in enumerate([(32, 512), (64, 256), (128, 128), (256, 64)]):
    x, P = T._block_inputs(c, (hw, hw), 1 + level, n=1)
    k = boxes[level]
    assert k[0] < hw and k[1] < hw and K.naf_tail_supported(c, hw * hw)

    def run():
        for _ in range(REP):
            out = E.naf_fwd_local(x, P, *k)
        return out
    prev = K.set_pack_plan(plan)
    try:
        switched(True, run)()
        switched(False, run)()
        plan.run()                                         # every pack of the block recorded and valid from here on
        ts = alternate(dict(fused=switched(True, run), per_op=switched(False, run)), a.rounds)
    finally:
        K.set_pack_plan(prev)
    us = {n: round(statistics.median(v) / REP * 1e3, 2) for n, v in ts.items()}
    blocks.append(dict(c=c, hw=hw, box=list(k), fused_us=us['fused'], per_op_us=us['per_op'],
                       fused_min_us=round(min(ts['fused']) / REP * 1e3, 2), per_op_min_us=round(min(ts['per_op']) / REP * 1e3, 2)))
    del x, P
res['blocks'] = blocks
write(res)

# ---- the error figures of the block test
errs = []
for math in ('bx3', 'hx2'):
    K.set_math(math)
    for c, hw, k in T.BLOCKS:
        x, P = T._block_inputs(c, hw, 100 + c)
        want = T.block64(x, P, *k)
        errs.append(dict(math=math, c=c, hw=list(hw), box=list(k), e_fused=float(f'{T._rel(T._local(x, P, k, True), want):.3e}'),
                         e_per_op=float(f'{T._rel(T._local(x, P, k, False), want):.3e}')))
K.set_math('bx3')
res['block_error_vs_float64'] = errs
write(res)

# ---- the whole network
NET = dict(type='NAFNetLocal', img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1],
           train_size=(1, 3, 256, 256))
net = define_network(dict(NET))
gen = torch.Generator().manual_seed(5)
with torch.no_grad():
    for name, p in net.named_parameters():
        if name.endswith(('beta', 'gamma')):
            p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
net = net.cuda()
img = torch.rand(1, 3, *a.hw, generator=gen).cuda()
fwd = dict(fused=switched(True, lambda: net(img)), per_op=switched(False, lambda: net(img)))
ts = alternate(fwd, a.rounds)
diff = (fwd['fused']() - fwd['per_op']()).abs().max().item()
pk = {n: [] for n in fwd}
for _ in range(2):
    for n, fn in fwd.items():
        pk[n].append(peak(fn))
res['network'] = dict(cfg={k: list(v) if isinstance(v, tuple) else v for k, v in NET.items()}, shape=[1, 3] + list(a.hw), ksizes=[list(k) for k in net.ksizes],
                      forward_ms={n: dict(median=round(statistics.median(v), 3), min=round(min(v), 3), max=round(max(v), 3)) for n, v in ts.items()},
                      peak_memory_MiB={n: round(max(v) / 2 ** 20, 1) for n, v in pk.items()},
                      max_abs_fused_minus_per_op=float(f'{diff:.3e}'))
write(res)
res['network']['kernels_per_forward'] = {n: kernels_of(fn) for n, fn in fwd.items()}
write(res)
print(json.dumps(res))
