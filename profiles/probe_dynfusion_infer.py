"""Inference of NAFNetDynamicFusion at the YAML-002 shape of 5k (width 32, enc [1,1,1,28], middle 1, dec [1,1,1,1]), bx3,
inputs 1 x 3 x 256^2 and 4 x 3 x 256^2.  One process, alternating runs, medians of device-event times:
  * peak memory above the resident state: the grad-enabled forward (the parent's code path, the baseline) against torch.no_grad();
  * whole-forward device time: grad-enabled | no-grad with the fused launches | no-grad with dynfusion_engine.INFER_KERNELS = False;
  * one block at each of the four fused channel counts (the shapes of the levels), the same three variants, microseconds;
  * each new launch on its own: microseconds and bytes per second on its algorithmic bytes (3 c-planes each: head reads x and writes
    t1, the stencil reads t1 and writes g, the tail reads g and x and writes out), back-to-back launches on the level's tensors.
Writes profiles/dynfusion_infer/probe_dynfusion_infer.json and prints it.   python profiles/probe_dynfusion_infer.py [out.json]"""
import gc
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from textualdegremoval_amd import dynfusion_engine as D, engine as E, kernels as K  # noqa: E402
from textualdegremoval_amd.kernels import PACK_FWD  # noqa: E402
from textualdegremoval_amd.models.archs import define_network  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'dynfusion_infer', 'probe_dynfusion_infer.json')
CFG = dict(img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1])
ROUNDS = 11


def timed(fn, rep):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(rep):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / rep


def alternate(fns, rep):
    """{name: median ms} of `fns` timed in turn, ROUNDS times, after two warm-up turns"""
    for _ in range(2):
        for f in fns.values():
            timed(f, rep)
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            t[k].append(timed(f, rep))
    return {k: statistics.median(v) for k, v in t.items()}, {k: min(v) for k, v in t.items()}


def peak_delta(fn):
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def with_switch(on, fn):
    def f():
        prev, D.INFER_KERNELS = D.INFER_KERNELS, on
        try:
            with torch.no_grad():
                return fn()
        finally:
            D.INFER_KERNELS = prev
    return f


def main():
    assert torch.cuda.is_available(), 'the probe measures on the GPU'
    K.set_math('bx3')
    torch.manual_seed(1)
    with torch.device('cuda'):
        net = define_network(dict(type='NAFNetDynamicFusion', **CFG))
    g = torch.Generator().manual_seed(2)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if p.dim() <= 1 or k.endswith(('beta', 'gamma')):
                p.add_((torch.randn(p.shape, generator=g) * 0.1).cuda())
    P = {k: p.detach() for k, p in net.named_parameters()}
    res = dict(probe='dynfusion_infer', cfg=CFG, math='bx3', device=torch.cuda.get_device_name(0), rounds=ROUNDS, inputs=[])
    for N in (1, 4):
        x = torch.rand(N, 3, 256, 256, device='cuda')
        kv = torch.randn(N, 10, 1024, device='cuda')
        fns = dict(grad_enabled=lambda: net(x, kv), no_grad_fused=with_switch(True, lambda: net(x, kv)),
                   no_grad_per_op=with_switch(False, lambda: net(x, kv)))
        for f in fns.values():
            f()
        mem = {k: peak_delta(f) / 2**20 for k, f in fns.items()}
        med, mn = alternate(fns, 3)
        a, b = fns['grad_enabled']().detach(), fns['no_grad_fused']()
        row = dict(N=N, H=256, W=256, peak_mib=mem, peak_ratio_no_grad_over_grad=mem['no_grad_fused'] / mem['grad_enabled'],
                   forward_ms_median=med, forward_ms_min=mn, max_abs_diff_fused_vs_grad_enabled=(a - b).abs().max().item(),
                   per_op_equals_grad_enabled=bool(torch.equal(a, fns['no_grad_per_op']())), blocks=[])
        del a, b
        # ---- one block of each fused level, its own projection table
        for lvl, c in enumerate((32, 64, 128, 256)):
            h = 256 >> lvl
            pre = f'encoders.{lvl}.layers.0.'
            Pb = E._sub(P, pre)
            xb = torch.randn(N, c, h, h, device='cuda')
            kvf = D.flat_kv(kv, N)
            _, Kt = D.proj_fwd(Pb, [('', c)], kvf)
            bf = dict(grad_enabled=lambda: D.dyn_naf_fwd(xb, Pb, Kt, 0), no_grad_fused=with_switch(True, lambda: D.dyn_naf_fwd(xb, Pb, Kt, 0, keep=False)),
                      no_grad_per_op=with_switch(False, lambda: D.dyn_naf_fwd(xb, Pb, Kt, 0, keep=False)))
            bmed, _ = alternate(bf, 10)
            # ---- the three launches on their own
            a0, b0, a1, b1, a2, b2 = D._slices(Kt, 0, c)
            w1p, w3p, w4p, w5p = (K.pack_weights(Pb[k], PACK_FWD)[0] for k in ('conv1.weight', 'conv3.weight', 'conv4.weight', 'conv5.weight'))
            t1 = K.dyn_head_infer(xb, a0, b0, Pb['norm1.weight'], Pb['norm1.bias'], E.LN_EPS, w1p, Pb['conv1.bias'])
            gg, pooled = K.dyn_dwsg_fwd(t1, Pb['conv2.weight'], Pb['conv2.bias'], a1, b1)
            s = K.sca_fwd(pooled, Pb['sca.1.weight'], Pb['sca.1.bias'])
            kf = dict(tdr_dyn_head_infer=lambda: K.dyn_head_infer(xb, a0, b0, Pb['norm1.weight'], Pb['norm1.bias'], E.LN_EPS, w1p, Pb['conv1.bias']),
                      tdr_dyn_dwsg_fwd=lambda: K.dyn_dwsg_fwd(t1, Pb['conv2.weight'], Pb['conv2.bias'], a1, b1),
                      tdr_dyn_tail_infer=lambda: K.dyn_tail_infer(gg, s, xb, w3p, Pb['conv3.bias'], Pb['beta'].view(-1), Pb['norm2.weight'], Pb['norm2.bias'],
                                                                  E.LN_EPS, w4p, Pb['conv4.bias'], a2, b2, w5p, Pb['conv5.bias'], Pb['gamma'].view(-1)))
            kmed, _ = alternate(kf, 20)
            plane = N * c * h * h * 4
            row['blocks'].append(dict(c=c, H=h, W=h, c_plane_bytes=plane, block_us={k: v * 1e3 for k, v in bmed.items()},
                                      kernels={k: dict(us=v * 1e3, algorithmic_bytes=3 * plane, tb_per_s=3 * plane / (v * 1e-3) / 1e12)
                                               for k, v in kmed.items()}))
        res['inputs'].append(row)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, 'w') as fh:
        json.dump(res, fh, indent=1)
        fh.write('\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
