"""The yardstick of SSIMLoss (csrc/tdr_ssim_loss.hip, losses.SSIMLoss): a torch restatement of the criterion -- three 1-D conv3d passes over
the [N,1,H,W,C] volume with replicate padding -- run under autograd in float64 (value, per-image SSIM, dpred) and once more in float32,
whose distance from the float64 run is the measure `e32` every gradient bar is made of (the rule of tests/_masa_ref.py: no bar is typed
in).  Also the explicit gradient formula with G^T built from the transposed filter matrices, the case table and the input builders."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from _masa_ref import bar, maxabs  # noqa: F401  (the tests take both from here)


def gauss11(dtype=torch.float64):
    x = torch.arange(11, dtype=torch.float64) - 5
    g = torch.exp(-(x * x) / (2 * 1.5 * 1.5))
    return (g / g.sum()).to(dtype)


def volume_filter(v, g):
    """v [N,C,H,W] -> G v as [N,H,W,C]: the 11-tap Gaussian along H, W and the channel axis, replicate borders on all three"""
    v = v.permute(0, 2, 3, 1)[:, None]
    for axis in (2, 3, 4):
        pad = [0] * 6
        pad[2 * (4 - axis)] = pad[2 * (4 - axis) + 1] = 5
        shape = [1] * 5
        shape[axis] = 11
        v = F.conv3d(F.pad(v, pad, mode='replicate'), g.view(shape))
    return v[:, 0]


def ssim_loss(pred, gt, w=1.0, max_value=1.0):
    """-> (loss, per-image SSIM [N]) in the dtype of pred"""
    g = gauss11(pred.dtype).to(pred.device)
    c1, c2 = (0.01 * max_value) ** 2, (0.03 * max_value) ** 2
    mu1, mu2 = volume_filter(pred, g), volume_filter(gt, g)
    s11 = volume_filter(pred * pred, g) - mu1 * mu1
    s22 = volume_filter(gt * gt, g) - mu2 * mu2
    s12 = volume_filter(pred * gt, g) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
    per = smap.flatten(1).mean(1)
    return w * (1 - per.mean()), per


def run(pred, gt, w, max_value, dtype):
    """value, per-image SSIM and dpred of the restatement under autograd in `dtype`"""
    p = pred.to(dtype).clone().requires_grad_(True)
    loss, per = ssim_loss(p, gt.to(dtype), w, max_value)
    loss.backward()
    return loss.detach(), per.detach(), p.grad.detach()


# ------------------------------------------------------------------------------------------------ the explicit formula
def filter_matrix(L):
    """[L, L] float64: row y holds the replicate-border 11-tap filter at position y of an axis of length L"""
    g = gauss11()
    m = torch.zeros(L, L, dtype=torch.float64)
    for y in range(L):
        for k in range(11):
            m[y, min(max(y + k - 5, 0), L - 1)] += g[k]
    return m


def adjoint_gather(p):
    """(G^T p) along the LAST axis in the gather form the kernel uses: the plain correlation, plus the taps rows 0..4 spend before row 0
    folded into row 0, plus the taps the last five rows spend past row L-1 folded into row L-1"""
    g = gauss11()
    L = p.shape[-1]
    out = torch.zeros_like(p)
    for x in range(L):
        for y in range(max(0, x - 5), min(L, x + 6)):
            out[..., x] += g[x - y + 5] * p[..., y]
    for y in range(min(5, L)):
        out[..., 0] += p[..., y] * g[:5 - y].sum()
    for y in range(max(0, L - 5), L):
        out[..., L - 1] += p[..., y] * g[6 + (L - 1 - y):].sum()
    return out


def dpred_formula(pred, gt, w, max_value, adjoint='matrix'):
    """float64 dpred = (-w / (N H W C)) [ G^T(dS/dmu1) + 2 pred G^T(dS/dE11) + gt G^T(dS/dE12) ], autograd-free.  adjoint 'matrix': G^T from
    the transposed filter matrices; 'gather': the fold form of adjoint_gather on every axis"""
    pred, gt = pred.double(), gt.double()
    N, C, H, W = pred.shape
    mats = [filter_matrix(L) for L in (H, W, C)]

    def G(v):                              # [N,C,H,W] -> [N,H,W,C]
        return torch.einsum('hy,wx,cj,njyx->nhwc', mats[0], mats[1], mats[2], v)

    def Gt(p):                             # [N,H,W,C] -> [N,C,H,W]
        if adjoint == 'matrix':
            return torch.einsum('hy,wx,cj,nhwc->njyx', mats[0], mats[1], mats[2], p)
        p = adjoint_gather(p)                                           # channel axis
        p = adjoint_gather(p.permute(0, 1, 3, 2)).permute(0, 1, 3, 2)   # W
        p = adjoint_gather(p.permute(0, 3, 2, 1)).permute(0, 3, 2, 1)   # H
        return p.permute(0, 3, 1, 2)
    c1, c2 = (0.01 * max_value) ** 2, (0.03 * max_value) ** 2
    mu1, mu2 = G(pred), G(gt)
    s11, s22, s12 = G(pred * pred) - mu1 * mu1, G(gt * gt) - mu2 * mu2, G(pred * gt) - mu1 * mu2
    a1, a2, b1, b2 = 2 * mu1 * mu2 + c1, 2 * s12 + c2, mu1 * mu1 + mu2 * mu2 + c1, s11 + s22 + c2
    S = a1 * a2 / (b1 * b2)
    dE11 = -S / b2
    dE12 = 2 * a1 / (b1 * b2)
    dmu1 = 2 * mu2 * a2 / (b1 * b2) - 2 * mu1 * S / b1 - 2 * mu1 * dE11 - mu2 * dE12
    return (-w / (N * H * W * C)) * (Gt(dmu1) + 2 * pred * Gt(dE11) + gt * Gt(dE12))


# ------------------------------------------------------------------------------------------------ cases
# shapes: the smallest that take every clamp and tail
SHAPES = [
    (1, 3, 1, 9),        # L = 1: both folds on one row
    (2, 1, 5, 7),        # shorter than the window radius on both axes, C = 1, two images
    (1, 3, 16, 16),      # exactly one tile
    (3, 3, 17, 33),      # one-pixel remainder tiles, three images
    (1, 1, 40, 24),      # several tiles, C = 1
    (2, 3, 64, 48),      # whole tiles only
]
KINDS = ('noise', 'smooth', 'flat')
CASES = [(s, k, 1.0) for s in SHAPES for k in KINDS]
CASES += [(s, k, 255.0) for s in ((3, 3, 17, 33), (1, 1, 40, 24)) for k in KINDS]
CASES += [((1, 2, 17, 9), 'noise', 1.0), ((1, 4, 17, 9), 'noise', 1.0)]
WEIGHT = 0.7             # a weight that is no power of two


def case_id(c):
    return 'x'.join(map(str, c[0])) + f'-{c[1]}-{int(c[2])}'


def make_inputs(shape, kind, max_value, seed=0):
    """-> (pred, gt) float32 [N,C,H,W]; pred = gt + 0.1 randn, not clamped; x max_value"""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(seed)
    if kind == 'noise':
        gt = torch.rand(N, C, H, W, generator=gen, dtype=torch.float64)
    elif kind == 'smooth':
        coarse = torch.rand(N, C, max(H // 8, 2), max(W // 8, 2), generator=gen, dtype=torch.float64)
        gt = F.interpolate(coarse, (H, W), mode='bilinear')
    else:
        gt = 0.5 + 1e-3 * torch.rand(N, C, H, W, generator=gen, dtype=torch.float64)
    pred = gt + 0.1 * torch.randn(N, C, H, W, generator=gen, dtype=torch.float64)
    return (pred * max_value).float(), (gt * max_value).float()


@functools.lru_cache(maxsize=None)
def reference(case):
    """computed once per case and shared (read-only): inputs, the float64 run, e32 of the float32 run"""
    shape, kind, max_value = case
    pred, gt = make_inputs(shape, kind, max_value)
    loss64, per64, d64 = run(pred, gt, WEIGHT, max_value, torch.float64)
    loss32, _, d32 = run(pred, gt, WEIGHT, max_value, torch.float32)
    return dict(pred=pred, gt=gt, loss64=loss64.item(), ssim64=per64, dpred64=d64, e32=maxabs(d32, d64),
                v32=abs(loss32.item() - loss64.item()))


def host_loss(ssim, w):
    """float32(double(float32 w) * (1.0 - (sum_n double(ssim[n])) / N)), n ascending: tdr_ssim_loss's definition of `loss`"""
    acc = 0.0
    for v in ssim.detach().cpu().numpy().astype(np.float64):
        acc += float(v)
    return np.float32(np.float64(np.float32(w)) * (1.0 - acc / ssim.numel()))
