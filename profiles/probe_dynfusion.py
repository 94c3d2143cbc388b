"""NAFNetDynamicFusion train step at the NAFNet shape of YAML 002 (width 64, enc [1,1,1,28], middle 1, dec [1,1,1,1]): the HIP step
(forward + backward + FusedClipAdamW), the two projection kernels on their own (time and GB/s on their algorithmic bytes), and the same
step with the reference-equivalent network in ATen fp32 eager (F.conv2d / F.linear, torch.optim.AdamW + clip_grad_norm_) on the same box.
Prints one JSON line.   python profiles/probe_dynfusion.py [N H W steps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from textualdegremoval_amd import dynfusion_engine as D, kernels as K  # noqa: E402
from textualdegremoval_amd.models.archs import define_network  # noqa: E402
from textualdegremoval_amd.optim import FusedClipAdamW  # noqa: E402

N, H, W, STEPS = (int(v) for v in (sys.argv[1:5] if len(sys.argv) >= 5 else (4, 256, 256, 5)))
CFG = dict(img_channel=3, width=64, middle_blk_num=1, enc_blk_nums=[1, 1, 1, 28], dec_blk_nums=[1, 1, 1, 1])


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


torch.manual_seed(1)
net = define_network(dict(type='NAFNetDynamicFusion', **CFG)).cuda()
x = torch.rand(N, 3, H, W, device='cuda')
gt = torch.rand(N, 3, H, W, device='cuda')
kv = torch.randn(N, 10, 1024, device='cuda')
n_proj = sum(p.numel() for k, p in net.named_parameters() if k.endswith(D.PROJ_SUFFIXES))
n_all = sum(p.numel() for p in net.parameters())
opt = FusedClipAdamW(net.parameters(), lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-4, max_norm=0.01)


def hip_step():
    opt.zero_grad(set_to_none=True)
    out = net(x, kv)
    loss, dpred = K.l1_loss(out.contiguous(), gt)
    out.backward(dpred)
    opt.step()


hip_ms = timed(hip_step, STEPS)

# ---- the projection kernels alone
P = {k: p.detach() for k, p in net.named_parameters()}
kvf = kv.view(N, -1)
tab, Kt = D.proj_fwd(P, D.block_prefixes(CFG), kvf)
dK = torch.randn_like(Kt)
fwd_ms = timed(lambda: K.kvproj_fwd(tab.tab, tab.nseg, tab.ntiles, kvf, tab.ld), 10)
grads = [torch.empty(sh, device='cuda') for sh in tab.shapes]
gtab = torch.tensor([t.data_ptr() for t in grads], dtype=torch.int64).cuda()
wgrad_ms = timed(lambda: K.kvproj_wgrad(tab.tab, gtab, tab.nseg, tab.ntiles, kvf, dK), 10)
dkv_ms = timed(lambda: K.kvproj_dkv(tab.tab, tab.nseg, tab.ntiles, dK, kvf.shape[1]), 10)
wbytes = 4 * n_proj
side = 4 * (kvf.numel() + Kt.numel())
del grads, gtab, dK, Kt
torch.cuda.synchronize()
opt = None
for p in net.parameters():
    p.grad = None
torch.cuda.empty_cache()


# ---- ATen fp32 eager, the reference's arithmetic restated functionally (tests/test_hip_dynfusion.py:_ref_net in fp32)
def ln(t, w, b):
    mu = t.mean(1, keepdim=True)
    var = (t - mu).pow(2).mean(1, keepdim=True)
    return (t - mu) / (var + 1e-6).sqrt() * w.view(1, -1, 1, 1) + b.view(1, -1, 1, 1)


def block(Q, pre, t, kf):
    c = t.shape[1]
    k0 = F.linear(kf, Q[pre + 'kernel.0.weight']).view(-1, 2 * c, 1, 1)
    u = ln(t * k0[:, :c] + k0[:, c:], Q[pre + 'norm1.weight'], Q[pre + 'norm1.bias'])
    u = F.conv2d(F.conv2d(u, Q[pre + 'conv1.weight'], Q[pre + 'conv1.bias']), Q[pre + 'conv2.weight'], Q[pre + 'conv2.bias'], padding=1,
                 groups=2 * c)
    k1 = F.linear(kf, Q[pre + 'sg1.kernel.0.weight']).view(-1, 4 * c, 1, 1)
    u = k1[:, :2 * c] * u + k1[:, 2 * c:]
    g = u[:, :c] * u[:, c:]
    g = g * F.conv2d(F.adaptive_avg_pool2d(g, 1), Q[pre + 'sca.1.weight'], Q[pre + 'sca.1.bias'])
    y = t + F.conv2d(g, Q[pre + 'conv3.weight'], Q[pre + 'conv3.bias']) * Q[pre + 'beta']
    u = F.conv2d(ln(y, Q[pre + 'norm2.weight'], Q[pre + 'norm2.bias']), Q[pre + 'conv4.weight'], Q[pre + 'conv4.bias'])
    k2 = F.linear(kf, Q[pre + 'sg2.kernel.0.weight']).view(-1, 4 * c, 1, 1)
    u = k2[:, :2 * c] * u + k2[:, 2 * c:]
    return y + F.conv2d(u[:, :c] * u[:, c:], Q[pre + 'conv5.weight'], Q[pre + 'conv5.bias']) * Q[pre + 'gamma']


def aten_net(Q, inp, kf):
    t = F.conv2d(inp, Q['intro.weight'], Q['intro.bias'], padding=1)
    skips = []
    for lvl, n in enumerate(CFG['enc_blk_nums']):
        for j in range(n):
            t = block(Q, f'encoders.{lvl}.layers.{j}.', t, kf)
        skips.append(t)
        t = F.conv2d(t, Q[f'downs.{lvl}.weight'], Q[f'downs.{lvl}.bias'], stride=2)
    for j in range(CFG['middle_blk_num']):
        t = block(Q, f'middle_blks.layers.{j}.', t, kf)
    for lvl, n in enumerate(CFG['dec_blk_nums']):
        t = F.pixel_shuffle(F.conv2d(t, Q[f'ups.{lvl}.0.weight']), 2) + skips[-1 - lvl]
        for j in range(n):
            t = block(Q, f'decoders.{lvl}.layers.{j}.', t, kf)
    return F.conv2d(t, Q['ending.weight'], Q['ending.bias'], padding=1) + inp


Q = {k: p.detach().clone().requires_grad_(True) for k, p in net.named_parameters()}
net = None
aopt = torch.optim.AdamW(list(Q.values()), lr=2e-4, betas=(0.9, 0.999), weight_decay=1e-4)


def aten_step():
    aopt.zero_grad(set_to_none=True)
    loss = F.l1_loss(aten_net(Q, x, kvf), gt)
    loss.backward()
    torch.nn.utils.clip_grad_norm_(list(Q.values()), 0.01)
    aopt.step()


aten_ms = timed(aten_step, STEPS)
print(json.dumps(dict(probe='dynfusion', N=N, H=H, W=W, cfg=CFG, params=n_all, proj_params=n_proj,
                      hip_step_ms=round(hip_ms, 3), aten_fp32_eager_step_ms=round(aten_ms, 3), speedup=round(aten_ms / hip_ms, 3),
                      kvproj_fwd_ms=round(fwd_ms, 4), kvproj_fwd_tbs=round((wbytes + side) / fwd_ms / 1e9, 3),
                      kvproj_wgrad_ms=round(wgrad_ms, 4), kvproj_wgrad_tbs=round((wbytes + side) / wgrad_ms / 1e9, 3),
                      kvproj_dkv_ms=round(dkv_ms, 4), kvproj_dkv_tbs=round((wbytes + side) / dkv_ms / 1e9, 3),
                      device=torch.cuda.get_device_name(0))))
