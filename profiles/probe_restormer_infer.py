"""The inference path of the Restormer family (restormer_engine.walk_fwd(keep=False): nothing saved, attn.project_out folded into the
per-image attention weights) against the grad-enabled forward -- the training forward, which a no-grad call also ran before the path
existed -- on the BASELINE configs[2] network (Restormer-ref dim 48, blocks [4, 6, 6, 8], 4 refinement blocks, fusion [2, 2, 2, 2]) at
1 x 3 x 256 x 256, one process, alternating runs:
  * peak memory above the resident state: grad-enabled | no-grad | no-grad with restormer_engine.INFER_FOLD = False, and the ratio;
  * whole-network time: the same three;
  * one TransformerBlock per level of the U-Net (C = 48 .. 384, and the 2C-wide level-0 fusion width): keep=True | keep=False with
    the fold | keep=False without it;
  * max |no-grad - grad-enabled| of the network output with the fold, on this network and on every case of
    tests/test_hip_restormer_inference.py in the three arithmetics (without the fold the two are bit-identical: asserted).
Writes profiles/restormer_infer/probe_restormer_infer.json (or `--out PATH`) and prints it.
python profiles/probe_restormer_infer.py [--out PATH] [--rounds R]"""
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
import torch  # noqa: E402

from oracle import nafnet_ref_oracle as NO, restormer_ref_oracle as RO  # noqa: E402
from textualdegremoval_amd import kernels as K, restormer_engine as R  # noqa: E402
from textualdegremoval_amd.models.archs import define_network  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'restormer_infer', 'probe_restormer_infer.json'))
ap.add_argument('--rounds', type=int, default=15)
ap.add_argument('--size', type=int, default=256)
a = ap.parse_args()
assert torch.cuda.is_available(), 'probe_restormer_infer.py measures on the GPU'
K.set_math('bx3')

KW = dict(dim=48, nf=48, num_blocks=[4, 6, 6, 8], num_refinement_blocks=4, heads=[1, 2, 4, 8], ext_n_blocks=[4, 4, 4, 4],
          reffusion_n_blocks=[2, 2, 2, 2])
cfg = RO.default_cfg(**KW)
net = define_network(dict(type='RestormerRefFusion', **cfg))
net.load_state_dict(RO.synth_params(cfg, seed=7), strict=True)
net = net.cuda()
lq, _, ref = NO.synth_pair(1, a.size, a.size, seed=77)
lq, ref = lq.cuda(), ref.cuda()


def train():
    return net(lq, ref)


def infer():
    with torch.no_grad():
        return net(lq, ref)


def infer_no_fold():
    prev, R.INFER_FOLD = R.INFER_FOLD, False
    try:
        return infer()
    finally:
        R.INFER_FOLD = prev


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


def summary(ts, unit='ms', scale=1.0):
    return {k: {f'median_{unit}': round(statistics.median(v) * scale, 3), f'min_{unit}': round(min(v) * scale, 3),
                f'max_{unit}': round(max(v) * scale, 3)} for k, v in ts.items()}


res = dict(probe='restormer_infer', device=torch.cuda.get_device_name(0), math=K.MATH, cfg=KW, shape=[1, 3, a.size, a.size], rounds=a.rounds)
out_train = train().detach()
assert torch.equal(infer_no_fold(), out_train)
res['max_abs_diff_fold_vs_grad_enabled'] = (infer() - out_train).abs().max().item()
first = peak(infer)
p_train, p_infer, p_nofold = peak(train), peak(infer), peak(infer_no_fold)
res['peak_memory_MiB'] = dict(grad_enabled=round(p_train / 2 ** 20, 1), no_grad=round(p_infer / 2 ** 20, 1),
                              no_grad_no_fold=round(p_nofold / 2 ** 20, 1), no_grad_first_measurement=round(first / 2 ** 20, 1))
res['peak_memory_ratio'] = round(p_infer / p_train, 4)
res['network_forward'] = summary(alternate(dict(grad_enabled=train, no_grad=infer, no_grad_no_fold=infer_no_fold), a.rounds, wall_ms))

# ---- one TransformerBlock per level: device time of a run of REP blocks between two events (weight packs cached in a PackPlan)
REP = 8
gen = torch.Generator().manual_seed(1)


def block_params(c, heads):
    h = int(c * 2.66)
    P = {}
    for nm, shp in [('norm1.body.weight', (c,)), ('norm1.body.bias', (c,)), ('attn.temperature', (heads, 1, 1)),
                    ('attn.qkv.weight', (3 * c, c, 1, 1)), ('attn.qkv_dwconv.weight', (3 * c, 1, 3, 3)), ('attn.project_out.weight', (c, c, 1, 1)),
                    ('norm2.body.weight', (c,)), ('norm2.body.bias', (c,)), ('ffn.project_in.weight', (2 * h, c, 1, 1)),
                    ('ffn.dwconv.weight', (2 * h, 1, 3, 3)), ('ffn.project_out.weight', (c, h, 1, 1))]:
        if len(shp) == 4:
            P[nm] = (torch.randn(shp, generator=gen) * (shp[1] * shp[2] * shp[3]) ** -0.5).cuda()
        else:
            P[nm] = (torch.randn(shp, generator=gen) * 0.2 + (0.0 if nm.endswith('bias') else 1.0)).cuda()
    return P


def dev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REP


blocks = []
for name, c, heads, hw in [('level 0 fusion block width (2C)', 96, 1, a.size), ('level 0', 48, 1, a.size), ('level 1', 96, 2, a.size // 2),
                           ('level 2', 192, 4, a.size // 4), ('level 3 (latent)', 384, 8, a.size // 8)]:
    P = block_params(c, heads)
    x = torch.randn(1, c, hw, hw, generator=gen).cuda()
    plan = K.PackPlan()                                    # the block's packs cached: the timed region is the block's own launches

    def run(keep, fold_on):
        def fn():
            prev, R.INFER_FOLD = R.INFER_FOLD, fold_on
            try:
                for _ in range(REP):
                    out, _ = R.tblock_fwd(x, P, heads, 'WithBias', keep=keep)
            finally:
                R.INFER_FOLD = prev
            return out
        return fn
    prev_plan = K.set_pack_plan(plan)
    try:
        want = run(True, True)()
        assert torch.equal(run(False, False)(), want)
        d = (run(False, True)() - want).abs().max().item()
        plan.run()
        ts = alternate(dict(keep=run(True, True), no_keep_fold=run(False, True), no_keep_no_fold=run(False, False)), a.rounds, dev_ms)
    finally:
        K.set_pack_plan(prev_plan)
    # the fold's own launches against the two it stands for: tdr_attn_fold_proj + batched re-pack + ONE per-image 1x1 convolution |
    # batched re-pack + per-image 1x1 convolution (attn v) + project_out (its pack cached, as in a training step)
    Gm = torch.randn(1, c, c, generator=gen).cuda()
    _, AT = K.mdta_softmax(Gm, (0.5 + torch.rand(1, 2 * c, generator=gen)).cuda(), P['attn.temperature'], heads)
    v = torch.randn(1, c, hw, hw, generator=gen).cuda()

    def rep(fn):
        def many():
            for _ in range(REP):
                fn()
        return many
    prev_plan = K.set_pack_plan(plan)
    try:
        tt = alternate(dict(fold_kernel=rep(lambda: K.attn_fold_proj(AT, P['attn.project_out.weight'], heads)),
                            tail_folded=rep(lambda: R.attn_tail_fwd(v, AT, P, heads, x, keep=False)),
                            tail_unfolded=rep(lambda: R.attn_tail_fwd(v, AT, P, heads, x, keep=True))), a.rounds, dev_ms)
    finally:
        K.set_pack_plan(prev_plan)
    blocks.append(dict(block=name, c=c, heads=heads, hw=hw, max_abs_diff_fold=d, **summary(ts, 'us', 1e3), attention_tail=summary(tt, 'us', 1e3)))
    del v, AT
    del x, P
res['blocks'] = blocks

# ---- the fold's effect on the output, per case of the test suite and arithmetic
import test_hip_restormer_inference as T  # noqa: E402

diffs = {}
for case in T.CASES:
    diffs[case] = {}
    for mode in T.MODES:
        out_t, out_nf, out_f, want = T._outputs(case, mode)
        assert torch.equal(out_nf, out_t), (case, mode)
        diffs[case][mode] = dict(fold_vs_grad_enabled=T.maxdiff(out_f, out_t),
                                 **({} if want is None else dict(fold_vs_reference=T.maxdiff(out_f, want), grad_enabled_vs_reference=T.maxdiff(out_t, want))))
res['max_abs_diff_per_case'] = diffs
res['max_abs_diff_fold_vs_grad_enabled_over_cases'] = {m: max(d[m]['fold_vs_grad_enabled'] for d in diffs.values()) for m in T.MODES}
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, 'w') as f:
    json.dump(res, f, indent=1)
    f.write('\n')
print(json.dumps(res))
