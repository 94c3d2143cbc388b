"""The inference path of NAFNetRefFusion (engine.net_fwd(keep=False): forward-only NAFBlock chains, nothing saved) against the
grad-enabled forward -- the training forward, which a no-grad call also ran before the path existed -- at the headline shape (width 32,
enc [1,1,1,28], 1 x 3 x 512 x 512), one process, alternating runs:
  * peak memory above the resident state of both forwards, and their ratio;
  * whole-network time: grad-enabled | no-grad | no-grad with engine.INFER_KERNELS = False (the training chains, their saved tensors
    dropped: what the walk's releases are worth without the kernels);
  * one NAFBlock per level of the U-Net (and the level-0 fusion block): engine.naf_fwd keep=True | keep=False, with the bytes the
    forward-only chains no longer write.
Writes profiles/infer/probe_infer.json (or `--out PATH`) and prints it.   python profiles/probe_infer.py [--out PATH] [--rounds R]"""
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

from oracle import nafnet_ref_oracle as O  # noqa: E402
from textualdegremoval_amd import engine as E, kernels as K  # noqa: E402
from textualdegremoval_amd.models.archs import define_network  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'infer', 'probe_infer.json'))
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--size', type=int, default=512)
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_infer.py measures on the GPU'

KW = dict(width=32, nf=32, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1], middle_blk_num=1, ext_n_blocks=[4, 4, 4, 4],
          reffusion_n_blocks=[2, 2, 2, 2, 2])
cfg = O.default_cfg(**KW)
net = define_network(dict(type='NAFNetRefFusion', **KW))
net.load_state_dict(O.synth_params(cfg, seed=7), strict=True)
net = net.cuda()
lq, _, ref = O.synth_pair(1, a.size, a.size, seed=77)
lq, ref = lq.cuda(), ref.cuda()


def train():
    return net(lq, ref)


def infer():
    with torch.no_grad():
        return net(lq, ref)


def infer_training_kernels():
    prev, E.INFER_KERNELS = E.INFER_KERNELS, False
    try:
        return infer()
    finally:
        E.INFER_KERNELS = prev


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


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) * 1e3
    del out
    return dt


def alternate(fns, rounds, timer):
    """{name: [ms per round]}: every round runs each variant once, in turn (same clocks, same neighbours on the host)"""
    for fn in fns.values():
        timer(fn)
        timer(fn)
    ts = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            ts[k].append(timer(fn))
    return ts


def summary(ts):
    return {k: dict(median_ms=round(statistics.median(v), 4), min_ms=round(min(v), 4), max_ms=round(max(v), 4)) for k, v in ts.items()}


res = dict(probe='infer', device=torch.cuda.get_device_name(0), math=K.MATH, cfg=KW, shape=[1, 3, a.size, a.size], rounds=a.rounds)
assert torch.equal(infer(), train().detach()) and torch.equal(infer_training_kernels(), infer())
first = peak(infer)
p_train, p_infer, p_infer_tk = peak(train), peak(infer), peak(infer_training_kernels)
res['peak_memory_MiB'] = dict(grad_enabled=round(p_train / 2 ** 20, 1), no_grad=round(p_infer / 2 ** 20, 1),
                              no_grad_training_kernels=round(p_infer_tk / 2 ** 20, 1), no_grad_first_measurement=round(first / 2 ** 20, 1))
res['peak_memory_ratio'] = round(p_infer / p_train, 4)
res['network_forward'] = summary(alternate(dict(grad_enabled=train, no_grad=infer, no_grad_training_kernels=infer_training_kernels),
                                           a.rounds, wall_ms))


# ---- one block per level: device time of a run of REP blocks between two events (weight packs cached in a PackPlan)
def block_params(c, gen):
    P = {}
    for nm, shp in [('beta', (1, c, 1, 1)), ('gamma', (1, c, 1, 1)), ('conv1.weight', (2 * c, c, 1, 1)), ('conv1.bias', (2 * c,)),
                    ('conv2.weight', (2 * c, 1, 3, 3)), ('conv2.bias', (2 * c,)), ('conv3.weight', (c, c, 1, 1)), ('conv3.bias', (c,)),
                    ('sca.1.weight', (c, c, 1, 1)), ('sca.1.bias', (c,)), ('conv4.weight', (2 * c, c, 1, 1)), ('conv4.bias', (2 * c,)),
                    ('conv5.weight', (c, c, 1, 1)), ('conv5.bias', (c,)), ('norm1.weight', (c,)), ('norm1.bias', (c,)),
                    ('norm2.weight', (c,)), ('norm2.bias', (c,))]:
        P[nm] = (torch.randn(shp, generator=gen) * 0.2 + (1.0 if nm in ('norm1.weight', 'norm2.weight') else 0.0)).cuda()
    return P


REP = 8
blocks = []
gen = torch.Generator().manual_seed(1)
plan = K.PackPlan()                                        # the blocks' packs cached: the timed region is the block's own launches
for name, c, hw, c_out in [('encoder level 0', 32, a.size, None), ('fusion level 0 (last: c_out = c / 2)', 64, a.size, 32),
                           ('encoder level 1', 64, a.size // 2, None), ('encoder level 2', 128, a.size // 4, None),
                           ('encoder level 3 (28 blocks)', 256, a.size // 8, None), ('middle (per-op launches)', 512, a.size // 16, None)]:
    P = block_params(c, gen)
    x = torch.randn(1, c, hw, hw, generator=gen).cuda()

    def run(keep):
        def fn():
            for _ in range(REP):
                out, _ = E.naf_fwd(x, P, c_out, keep=keep)
            return out
        return fn

    def dev_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REP
    prev = K.set_pack_plan(plan)
    try:
        run(True)()
        run(False)()
        plan.run()                                         # every pack of the block recorded and valid from here on
        ts = alternate(dict(keep=run(True), no_keep=run(False)), a.rounds, dev_ms)
    finally:
        K.set_pack_plan(prev)
    fused = K.naf_tail_supported(c, hw * hw, c_out) and K.naf_tail_supported(c, hw * hw)
    plane = 4 * c * hw * hw
    blocks.append(dict(block=name, c=c, hw=hw, c_out=c_out or c, fused_chains=bool(fused), **summary(ts),
                       # xn (head); y, yn, t4 = 2c (tail); the four statistics vectors
                       bytes_not_written=(5 * plane + 4 * 4 * hw * hw) if fused else 0))
    del x, P
res['blocks'] = blocks
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
