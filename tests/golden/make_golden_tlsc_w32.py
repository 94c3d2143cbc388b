"""Generate the golden vector of the fused TLSC path (tests/test_hip_tlsc_fused.py) by running the REFERENCE on CPU.

Run in the build container only:   python tests/golden/make_golden_tlsc_w32.py
Writes tests/golden/tlsc_w32.npz (data only): `NAFNetLocal` of models/archs/network_nafnet_guided_arch.py:756-768 at width 32 with one
encoder level, so that both channel counts it meets (32 at level 0, 64 in the middle) are ones the fused NAFBlock chains take, run on
a 63 x 95 image whose padded levels (64 x 96 -> HW 6144, 32 x 48 -> HW 1536) are multiples of the chains' 64-pixel tile and larger than the
pooling boxes (48 x 48, 24 x 24): every block pools locally.  Weights stored.  Seeds and the perturbation of the 1-D / beta / gamma
parameters are those of make_golden_tlsc.py (a freshly constructed NAFNet has beta = gamma = 0: every block would be the identity).
The three-level variant is 1.17 MB, over the limit for a committed file; C = 128 / 256 are tested at block level."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_tlsc import import_ref  # noqa: E402


def naflocal_w32_case(d):
    naf = import_ref('network_nafnet_guided_arch')
    torch.manual_seed(7)
    net = naf.NAFNetLocal(img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=[1], dec_blk_nums=[1], train_size=(1, 3, 32, 32))
    g = torch.Generator().manual_seed(8)
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.add_(torch.randn(p.shape, generator=g) * 0.1 if p.dim() <= 1 or k.endswith(('beta', 'gamma')) else 0)
    ks = [tuple(m.kernel_size) for m in net.modules() if isinstance(m, sys.modules['models.archs.nafnet_local_arch'].AvgPool2d)]
    x = torch.rand(1, 3, 63, 95, generator=g)                  # padded to 64 x 96 (one encoder level: multiples of 2)
    with torch.no_grad():
        out = net(x)
        out64 = net.double()(x.double())
    d['x'], d['out'], d['ksizes'] = x.numpy(), out.numpy(), np.array(ks)
    d['names'] = np.array([k for k, _ in net.named_parameters()])
    for k, p in net.float().named_parameters():
        d['p_' + k] = p.detach().numpy()
    print('NAFNetLocal w32', tuple(out.shape), float(out.abs().mean()), ks, 'float32 vs float64', float((out.double() - out64).abs().max()))


if __name__ == '__main__':
    d = {}
    naflocal_w32_case(d)
    path = os.path.join(HERE, 'tlsc_w32.npz')
    np.savez_compressed(path, **d)
    print('wrote tlsc_w32.npz', len(d), 'arrays', os.path.getsize(path), 'bytes')
