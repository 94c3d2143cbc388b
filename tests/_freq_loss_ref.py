"""The yardstick of FFTLoss (csrc/tdr_freq_loss.hip, losses.FFTLoss): the criterion on d = float32(pred - target) as torch.fft under
autograd, in float64 (the truth: value, dpred, spectrum) and once more in float32, whose distance from the float64 run is what every bar of
tests/test_hip_freq_loss.py is made of (the rule of tests/_masa_ref.py: no bar is typed in).  Also the closed-form gradient of
include/tdr.h, the literal two-tensor expression, the case table with its searched seeds, and the margin condition: in every case the
smallest |Re| or |Im| of the float64 spectrum (the structurally zero imaginary parts of the self-conjugate bins left out) is at least
16 x the largest spectrum error of the float32 run, so no sign decision is within reach of a kernel that meets the spectrum bar."""
import functools
import math

import numpy as np
import torch

from _masa_ref import ULP32, bar, maxabs  # noqa: F401  (the tests take them from here)


def takes(L):
    """the admissible transform lengths restated: m * 2^a, m in {1, 3, 5}, a >= 2, 4 <= L <= 1024"""
    if not 4 <= L <= 1024:
        return False
    a = 0
    while L % 2 == 0:
        L //= 2
        a += 1
    return a >= 2 and L in (1, 3, 5)


def literal(pred, gt, w=1.0, onesided=False):
    """the expression of the SFNet / MIMO-UNet recipes (fft2) and of the BasicSR forks (rfft2), on the two tensors"""
    fft = torch.fft.rfft2 if onesided else torch.fft.fft2
    fp, fg = fft(pred), fft(gt)
    return w * (torch.stack([fp.real, fp.imag], -1) - torch.stack([fg.real, fg.imag], -1)).abs().mean()


def kx_weights(W, onesided, dtype=torch.float64):
    """-> (c, m, count per plane row): the value weights c[kx], the gradient weights m[kx] on the half spectrum"""
    edge = torch.zeros(W // 2 + 1, dtype=torch.bool)
    edge[0] = edge[W // 2] = True
    one = torch.ones(W // 2 + 1, dtype=dtype)
    if onesided:
        return one, torch.where(edge, one, 0.5 * one), W // 2 + 1
    return torch.where(edge, one, 2 * one), one, W


def half_spectrum(d):
    """D on kx in [0, W/2], the imaginary parts of the four self-conjugate bins exactly 0"""
    H, W = d.shape[-2:]
    D = torch.fft.rfft2(d)
    re, im = D.real.clone(), D.imag.clone()
    for ky in (0, H // 2):
        for kx in (0, W // 2):
            im[..., ky, kx] = 0
    return re, im


def closed_form(d, w=1.0, onesided=False):
    """d [N,C,H,W] (any float dtype) -> (loss, dpred, spec [P,H,W/2+1,2]) by the formulas of include/tdr.h, autograd-free"""
    N, C, H, W = d.shape
    P = N * C
    c, m, cols = kx_weights(W, onesided, d.dtype)
    count = 2 * P * H * cols
    re, im = half_spectrum(d)
    loss = w * (c * (re.abs() + im.abs())).sum() / count
    gh = torch.complex(m * torch.sign(re), m * torch.sign(im))
    dpred = (w / count) * torch.fft.irfft2(gh, s=(H, W), norm='forward')
    return loss, dpred, torch.stack([re, im], -1).reshape(P, H, W // 2 + 1, 2)


def run(d32, w, onesided, dtype):
    """value and dpred of the criterion on d under autograd in `dtype` (target = 0: the transform is linear), and the spectrum"""
    d = d32.to(dtype).clone().requires_grad_(True)
    loss = literal(d, torch.zeros_like(d), w, onesided)
    loss.backward()
    re, im = half_spectrum(d.detach())
    return loss.detach(), d.grad.detach(), torch.stack([re, im], -1).reshape(-1, d.shape[2], d.shape[3] // 2 + 1, 2)


# ------------------------------------------------------------------------------------------------ cases
# (shape, seed, weight): the smallest shapes at which each path can go wrong; the seed of each is the first of 0, 1, 2, ... whose margin
# holds (tests/test_freq_loss_reference.py asserts it for every case)
CASES = [
    ((1, 1, 4, 4), 0, 1.0),          # smallest admissible size
    ((2, 3, 8, 8), 0, 1.0),          # small, several planes
    ((1, 3, 16, 48), 0, 1.0),        # radix 3 along W
    ((1, 3, 48, 16), 1, 0.1),        # radix 3 along H
    ((1, 1, 40, 32), 0, 1.0),        # radix 5 along H
    ((1, 2, 32, 40), 0, 1.0),        # radix 5 along W
    ((3, 4, 12, 20), 0, 0.7),        # both odd radices, several planes
    ((2, 3, 64, 64), 0, 1.0),        # mid size
    ((1, 1, 1024, 8), 0, 1.0),       # longest line along H (the 8-column tile)
    ((1, 1, 8, 1024), 0, 1.0),       # longest line along W
    ((1, 3, 128, 256), 0, 0.1),      # rectangular
    ((1, 3, 256, 256), 1, 1.0),      # realistic patch
]
MODES = (False, True)                # onesided
RUNS = [(c, o) for c in CASES for o in MODES]


def case_id(c):
    return 'x'.join(map(str, c[0])) + f'-s{c[1]}-w{c[2]}'


def run_id(r):
    return case_id(r[0]) + ('-one' if r[1] else '-two')


def make_inputs(shape, seed):
    """pred = rand, gt = clamp(pred + 0.1 randn, 0, 1), float32"""
    gen = torch.Generator().manual_seed(seed)
    pred = torch.rand(*shape, generator=gen, dtype=torch.float32)
    gt = (pred + 0.1 * torch.randn(*shape, generator=gen, dtype=torch.float32)).clamp(0, 1)
    return pred, gt


def margin(spec64):
    """the smallest |Re| or |Im| over all bins, without the imaginary parts of the self-conjugate bins"""
    H, WP = spec64.shape[1:3]
    a = spec64.abs().clone()
    for ky in (0, H // 2):
        for kx in (0, WP - 1):
            a[:, ky, kx, 1] = math.inf
    return a.min().item()


@functools.lru_cache(maxsize=None)
def reference(case, onesided):
    """computed once per run and shared (read-only)"""
    shape, seed, w = case
    pred, gt = make_inputs(shape, seed)
    d32 = pred - gt                                   # one float32 subtraction: the definition
    loss64, d64, spec64 = run(d32, w, onesided, torch.float64)
    loss32, dp32, spec32 = run(d32, w, onesided, torch.float32)
    return dict(pred=pred, gt=gt, d32=d32, loss64=loss64.item(), dpred64=d64, spec64=spec64,
                v32=abs(loss32.item() - loss64.item()), e32=maxabs(dp32, d64), s32=maxabs(spec32, spec64), mgn=margin(spec64))


def ulp_bar(x32err, ref_top):
    """max(8 x the float32 reference's error, 4 float32 ulp of the reference's magnitude)"""
    return max(8 * x32err, 4 * ULP32 * abs(ref_top))


def loss_from_spec(spec, W, w, onesided):
    """the value from a spectrum [P,H,W/2+1,2] by the closed form, in float64"""
    c, _, cols = kx_weights(W, onesided)
    P, H = spec.shape[:2]
    s = spec.double().abs()
    return w * (c[None, None, :] * (s[..., 0] + s[..., 1])).sum().item() / (2 * P * H * cols)


def np32(x):
    return np.float32(x)
