"""Generate golden vectors for NAFNetDynamicFusion (models/archs/network_nafnet_guided_diffir_arch.py:237-544, the text-embedding
modulated NAFNet) by running the REFERENCE classes on CPU.

Run in the build container only:   python tests/golden/make_golden_dynfusion.py
Writes tests/golden/dynfusion.npz (data only).  The projection weights (`kernel.0.weight`, `sg1.kernel.0.weight`,
`sg2.kernel.0.weight`: 85 MB at width 8) are NOT stored: `draw_proj` draws them from numpy.random.default_rng(seed), uniform in
+-1/sqrt(10240) (nn.Linear's default bound), and tests/test_hip_dynfusion.py draws them the same way.  So are the inputs (`draw_inputs`).
Every other parameter is the reference's default init under torch.manual_seed plus N(0, 0.1) on the 1-D tensors and beta / gamma (no
block is an identity) and is stored.  For each projection the gradient with respect to its OUTPUT (`dk`, captured with a hook) is
stored: its weight gradient is dk^T kv.
Cases: (a) width 8, enc [1,1,2], middle 1, dec [1,1,1], 2x3x64x64; (b) the same net on 2x3x60x44 (zero-padded to 64x48);
(c) three train steps of (a) as the DiffIR model takes them (image_restoration_text_embed_diffir_model.py:345-373: L1,
clip_grad_norm_(0.01), AdamW lr 2e-4 / wd 1e-4); (d) the error strings of defects R10 (a Mapper(num_words=20) embedding) and R11
(NAFNetLocalDynamic)."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
CFG = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 2], dec_blk_nums=[1, 1, 1])
PROJ = ('kernel.0.weight', 'sg1.kernel.0.weight', 'sg2.kernel.0.weight')


def is_proj(name):
    return name.endswith(PROJ)


def draw_proj(names_shapes, seed):
    """the projection weights, in registration order: uniform in +-1/sqrt(10240), float32"""
    rng = np.random.default_rng(seed)
    bound = 1.0 / np.sqrt(10240.0)
    return {k: rng.uniform(-bound, bound, size=sh).astype(np.float32) for k, sh in names_shapes if is_proj(k)}


def draw_inputs(seed, N, H, W):
    """image [N,3,H,W] in [0,1), k_v [N,10,1024] ~ N(0,1), target [N,3,H,W], output cotangent [N,3,H,W] ~ N(0,1)"""
    rng = np.random.default_rng(seed)
    x = rng.random((N, 3, H, W), dtype=np.float32)
    kv = rng.standard_normal((N, 10, 1024), dtype=np.float32)
    gt = rng.random((N, 3, H, W), dtype=np.float32)
    go = rng.standard_normal((N, 3, H, W), dtype=np.float32)
    return x, kv, gt, go


def import_ref(name):
    sys.path.insert(0, REF)
    m = types.ModuleType('models'); m.__path__ = [REF + '/models']; sys.modules['models'] = m
    a = types.ModuleType('models.archs'); a.__path__ = [REF + '/models/archs']; sys.modules['models.archs'] = a
    return importlib.import_module('models.archs.' + name)


def build(mod, d):
    torch.manual_seed(11)
    net = mod.NAFNetDynamicFusion(**CFG)
    g = torch.Generator().manual_seed(12)
    names = [(k, tuple(p.shape)) for k, p in net.named_parameters()]
    proj = draw_proj(names, seed=13)
    with torch.no_grad():
        for k, p in net.named_parameters():
            if is_proj(k):
                p.copy_(torch.from_numpy(proj[k]))
            elif p.dim() <= 1 or k.endswith(('beta', 'gamma')):
                p.add_(torch.randn(p.shape, generator=g) * 0.1)
    d['names'] = np.array([k for k, _ in names])
    d['shapes'] = np.array([str(list(s)) for _, s in names])
    for k, p in net.named_parameters():
        if not is_proj(k):
            d['p_' + k] = p.detach().numpy().copy()
    return net


def hooks(net, store):
    hs = []
    for mname, m in net.named_modules():
        if isinstance(m, torch.nn.Linear):
            def fwd(mod, inp, out, mname=mname):
                out.register_hook(lambda gr, mname=mname: store.__setitem__(mname, gr.detach().clone()))
            hs.append(m.register_forward_hook(fwd))
    return hs


def run_case(net, tag, seed, N, H, W, d):
    x, kv, _, go = draw_inputs(seed, N, H, W)
    xt = torch.from_numpy(x).requires_grad_(True)
    kvt = torch.from_numpy(kv).requires_grad_(True)
    dks = {}
    hs = hooks(net, dks)
    net.zero_grad()
    out = net(xt, kvt)
    (out * torch.from_numpy(go)).sum().backward()
    for h in hs:
        h.remove()
    d[tag + '_out'], d[tag + '_gx'], d[tag + '_gkv'] = out.detach().numpy(), xt.grad.numpy(), kvt.grad.numpy()
    for mname, gr in dks.items():
        d[f'{tag}_dk_{mname}.weight'] = gr.numpy()
    d[tag + '_gnorm'] = np.array([p.grad.double().norm().item() for _, p in net.named_parameters()])
    d[tag + '_gmax'] = np.array([p.grad.abs().max().item() for _, p in net.named_parameters()])
    print(tag, tuple(out.shape), float(out.abs().mean()), len(dks))


def trajectory(mod, d):
    net = build(mod, {})
    x, kv, gt, _ = draw_inputs(21, 2, 64, 64)
    opt = torch.optim.AdamW(net.parameters(), lr=2e-4, weight_decay=1e-4, betas=(0.9, 0.999))
    losses = []
    for _ in range(3):
        opt.zero_grad()
        out = net(torch.from_numpy(x), torch.from_numpy(kv))
        loss = torch.nn.functional.l1_loss(out, torch.from_numpy(gt))
        loss.backward()
        torch.nn.utils.clip_grad_norm_(net.parameters(), 0.01)
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        out = net(torch.from_numpy(x), torch.from_numpy(kv))
    d['traj_losses'] = np.array(losses)
    d['traj_psum'] = np.array([p.detach().double().sum().item() for p in net.parameters()])
    d['traj_final_out'] = out.numpy()
    print('trajectory', losses)


def defects(mod, d):
    net = mod.NAFNetDynamicFusion(**CFG)
    try:
        net(torch.rand(1, 3, 32, 32), torch.randn(1, 20, 1024))
        d['r10_error'] = np.array('')
    except RuntimeError as e:
        d['r10_error'] = np.array(str(e))
    try:
        mod.NAFNetLocalDynamic(**CFG, train_size=(1, 3, 32, 32))
        d['r11_error'] = np.array('')
    except TypeError as e:
        d['r11_error'] = np.array(str(e))
    print('R10:', d['r10_error'], '| R11:', d['r11_error'])


def main():
    mod = import_ref('network_nafnet_guided_diffir_arch')
    d = {}
    net = build(mod, d)
    run_case(net, 'a', 1, 2, 64, 64, d)
    run_case(net, 'b', 2, 2, 60, 44, d)
    trajectory(mod, d)
    defects(mod, d)
    np.savez_compressed(os.path.join(HERE, 'dynfusion.npz'), **d)


if __name__ == '__main__':
    main()
