"""Pixel losses with the reference's names (losses/losses.py:26-122).  On the device every criterion with mean reduction is
the HIP kernel tdr_pixel_loss (value + gradient in one pass); `step_kind()` tells the train step which one to fuse.  The
torch expressions below serve host tensors and the weighted / 'none' / 'sum' variants no shipped YAML selects.

SSIMLoss is the project's own criterion (the reference trains on none): w * (1 - mean_n SSIM_n) with SSIM_n the validation metric's 11^3
Gaussian SSIM over the [H,W,C] volume (metrics/psnr_ssim.py:131-176) at a FIXED max_value.  On the device it is the HIP kernel
tdr_ssim_loss (value, and the gradient through the adjoint of the replicate-border filter); its `step_kind()` is (LOSS_SSIM, weight,
max_value) and the train step fuses it alone (`pixel_opt`) or next to a pixel criterion (`ssim_opt`).  It has no ATen path on the device.

FFTLoss is the frequency-domain L1 term SFNet / MIMO-UNet (`L1 + 0.1 FFTLoss`, at three scales) and the BasicSR forks (DeepRFT's rfft2
form: onesided=True) are trained with: w * mean |stack(Re, Im)(fft2(pred) - fft2(target))|.  On the device it is the HIP kernel
tdr_freq_loss -- a hand-written 2-D real FFT for lengths m 2^a, m in {1, 3, 5}, 4 ... 1024, value and gradient; its `step_kind()` is
(LOSS_FREQ, weight, onesided) and the train step fuses it alone (`pixel_opt`) or next to the other criteria (`freq_opt`).  Host tensors
take the literal torch.fft expression; on the device it has no ATen path either."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from .. import kernels as K

_reduction_modes = ['none', 'mean', 'sum']


class _PixFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, kind, loss_weight, eps):
        loss, dpred = K.pixel_loss(kind, pred.contiguous(), target.contiguous(), loss_weight, eps)
        ctx.save_for_backward(dpred)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None, None


def _weight_reduce(loss, weight, reduction):
    """losses/loss_util.py:25-54 (weight_reduce_loss): element-wise weight, then the reduction; the weighted mean divides by
    the weight mass -- weight.sum() for a per-channel weight, weight.sum() * C for a one-channel weight (no clamp)."""
    if weight is not None:
        assert weight.dim() == loss.dim()
        assert weight.size(1) == 1 or weight.size(1) == loss.size(1)
        loss = loss * weight
    if weight is None or reduction == 'sum':
        return loss.mean() if reduction == 'mean' else (loss.sum() if reduction == 'sum' else loss)
    if reduction == 'mean':
        return loss.sum() / (weight.sum() if weight.size(1) > 1 else weight.sum() * loss.size(1))
    return loss


def _on_device(pred, target):
    return pred.is_cuda and pred.dim() == 4 and pred.dtype == torch.float32 and target.dtype == torch.float32


class L1Loss(nn.Module):
    def __init__(self, loss_weight=1.0, reduction='mean'):
        super().__init__()
        if reduction not in _reduction_modes:
            raise ValueError(f'Unsupported reduction mode: {reduction}. Supported ones are: {_reduction_modes}')
        self.loss_weight = loss_weight
        self.reduction = reduction

    def forward(self, pred, target, weight=None, **kwargs):
        if _on_device(pred, target) and weight is None and self.reduction == 'mean':
            return _PixFn.apply(pred, target, K.LOSS_L1, float(self.loss_weight), 0.0)
        return self.loss_weight * _weight_reduce((pred - target).abs(), weight, self.reduction)

    def step_kind(self):
        return (K.LOSS_L1, float(self.loss_weight), 0.0) if self.reduction == 'mean' else None


class MSELoss(nn.Module):
    def __init__(self, loss_weight=1.0, reduction='mean'):
        super().__init__()
        if reduction not in _reduction_modes:
            raise ValueError(f'Unsupported reduction mode: {reduction}. Supported ones are: {_reduction_modes}')
        self.loss_weight = loss_weight
        self.reduction = reduction

    def forward(self, pred, target, weight=None, **kwargs):
        if _on_device(pred, target) and weight is None and self.reduction == 'mean':
            return _PixFn.apply(pred, target, K.LOSS_MSE, float(self.loss_weight), 0.0)
        return self.loss_weight * _weight_reduce((pred - target) ** 2, weight, self.reduction)

    def step_kind(self):
        return (K.LOSS_MSE, float(self.loss_weight), 0.0) if self.reduction == 'mean' else None


class PSNRLoss(nn.Module):
    def __init__(self, loss_weight=1.0, reduction='mean', toY=False):
        super().__init__()
        assert reduction == 'mean'
        self.loss_weight, self.scale, self.toY = loss_weight, 10 / np.log(10), toY

    def step_kind(self):
        return (K.LOSS_PSNR_Y if self.toY else K.LOSS_PSNR, float(self.loss_weight), 0.0)

    def forward(self, pred, target):
        assert len(pred.size()) == 4
        if _on_device(pred, target) and (not self.toY or pred.shape[1] == 3):
            return _PixFn.apply(pred, target, *self.step_kind())
        if self.toY:
            coef = torch.tensor([65.481, 128.553, 24.966], device=pred.device).reshape(1, 3, 1, 1)
            pred = ((pred * coef).sum(dim=1, keepdim=True) + 16.) / 255.
            target = ((target * coef).sum(dim=1, keepdim=True) + 16.) / 255.
        return self.loss_weight * self.scale * torch.log(((pred - target) ** 2).mean(dim=(1, 2, 3)) + 1e-8).mean()


class _SsimFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, loss_weight, max_value):
        loss, _, dpred = K.ssim_loss(pred.contiguous(), target.contiguous(), loss_weight, max_value)
        ctx.save_for_backward(dpred)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None


def _ssim_volume_filter(v, g):
    """v [N,C,H,W] -> the 11-tap Gaussian along H, W and the channel axis of the [H,W,C] volume, replicate borders on all three"""
    v = v.permute(0, 2, 3, 1).unsqueeze(1)               # [N,1,H,W,C]
    for axis in (2, 3, 4):
        pad = [0] * 6
        pad[2 * (4 - axis)] = pad[2 * (4 - axis) + 1] = 5
        shape = [1] * 5
        shape[axis] = 11
        v = F.conv3d(F.pad(v, pad, mode='replicate'), g.view(shape))
    return v.squeeze(1)


class SSIMLoss(nn.Module):
    """w * (1 - mean over images of SSIM_n): SSIM_n the mean of the SSIM map of the [H,W,C] volume under the 11^3 Gaussian window
    (sigma 1.5, replicate borders) -- calculate_ssim's arithmetic with C1 = (0.01 max_value)^2, C2 = (0.03 max_value)^2 at the FIXED
    max_value given here (the metric's `1 if max <= 1 else 255` would put a jump into a criterion).  pred receives the gradient."""

    def __init__(self, loss_weight=1.0, reduction='mean', max_value=1.0):
        super().__init__()
        assert reduction == 'mean'
        self.loss_weight, self.max_value = loss_weight, max_value

    def step_kind(self):
        return (K.LOSS_SSIM, float(self.loss_weight), float(self.max_value))

    def forward(self, pred, target):
        if pred.is_cuda or target.is_cuda:
            if not (_on_device(pred, target) and target.is_cuda and pred.shape == target.shape and 1 <= pred.shape[1] <= 4):
                raise ValueError(f'SSIMLoss on the device takes float32 [N,C,H,W] tensors of one shape with C <= 4 (tdr_ssim_loss), not '
                                 f'pred {tuple(pred.shape)} {pred.dtype} / target {tuple(target.shape)} {target.dtype}')
            return _SsimFn.apply(pred, target, float(self.loss_weight), float(self.max_value))
        assert pred.dim() == 4 and pred.shape == target.shape
        x = torch.arange(11, dtype=torch.float64) - 5
        g = torch.exp(-(x * x) / (2 * 1.5 * 1.5))
        g = (g / g.sum()).to(pred.dtype)
        c1, c2 = (0.01 * self.max_value) ** 2, (0.03 * self.max_value) ** 2
        mu1, mu2 = _ssim_volume_filter(pred, g), _ssim_volume_filter(target, g)
        s11 = _ssim_volume_filter(pred * pred, g) - mu1 * mu1
        s22 = _ssim_volume_filter(target * target, g) - mu2 * mu2
        s12 = _ssim_volume_filter(pred * target, g) - mu1 * mu2
        smap = ((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s11 + s22 + c2))
        return self.loss_weight * (1 - smap.flatten(1).mean(1).mean())


class _FreqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, loss_weight, onesided):
        # (no gradient asked for -- a criterion evaluated for its value: the value-only launches, the same loss bits)
        loss, dpred = K.freq_loss(pred.contiguous(), target.contiguous(), loss_weight, onesided, want_grad=ctx.needs_input_grad[0])
        if dpred is not None:
            ctx.save_for_backward(dpred)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (dpred,) = ctx.saved_tensors
        return dpred * g, None, None, None


class FFTLoss(nn.Module):
    """w * mean |stack(fft2(pred).real, fft2(pred).imag) - stack(fft2(target).real, fft2(target).imag)| over the last two axes (the SFNet /
    MIMO-UNet term); onesided=True takes rfft2 instead (the BasicSR forks).  On the device: tdr_freq_loss, for H and W each m 2^a with m
    in {1, 3, 5}, a >= 2, 4 ... 1024 -- other sizes are refused, never padded (padding changes the criterion).  pred receives the gradient."""

    def __init__(self, loss_weight=1.0, reduction='mean', onesided=False):
        super().__init__()
        assert reduction == 'mean'
        self.loss_weight, self.onesided = loss_weight, bool(onesided)

    def step_kind(self):
        return (K.LOSS_FREQ, float(self.loss_weight), float(self.onesided))

    def forward(self, pred, target):
        if pred.is_cuda or target.is_cuda:
            if not (_on_device(pred, target) and target.is_cuda and pred.shape == target.shape
                    and K.freq_loss_takes(pred.shape[2], pred.shape[3])):
                raise ValueError(f'FFTLoss on the device takes float32 [N,C,H,W] tensors of one shape with {K.FREQ_LENGTHS} '
                                 f'(tdr_freq_loss), not pred {tuple(pred.shape)} {pred.dtype} / target {tuple(target.shape)} {target.dtype}')
            return _FreqFn.apply(pred, target, float(self.loss_weight), self.onesided)
        assert pred.dim() == 4 and pred.shape == target.shape
        fft = torch.fft.rfft2 if self.onesided else torch.fft.fft2
        fp, ft = fft(pred), fft(target)
        return self.loss_weight * (torch.stack([fp.real, fp.imag], -1) - torch.stack([ft.real, ft.imag], -1)).abs().mean()


class CharbonnierLoss(nn.Module):
    def __init__(self, loss_weight=1.0, reduction='mean', eps=1e-3):
        super().__init__()
        self.eps = eps
        self.loss_weight, self.reduction = loss_weight, reduction      # stored for the step; the value ignores both (reference :114-122)

    def step_kind(self):
        return (K.LOSS_CHARBONNIER, 1.0, float(self.eps))

    def forward(self, x, y):
        if _on_device(x, y):
            return _PixFn.apply(x, y, *self.step_kind())
        diff = x - y
        return torch.mean(torch.sqrt(diff * diff + self.eps * self.eps))
