"""A numpy restatement of the contract of tdr_val_metrics (include/tdr.h): quantise, crop, the integer squared error / largest byte /
count, and the Y plane by the explicit order of operations.  Shared by test_val_metrics_host.py and test_hip_val_metrics.py."""
import numpy as np
import torch

COLS = dict(S=0, MAX=1, COUNT=2, SSIM3D=3, SY=4, COUNT_Y=5, SSIMY=6)
LUT = np.arange(256, dtype=np.float32) / np.float32(255.)                                # float32(u) / 255, numpy's division


def quantise(x, swap_rb):
    """one operand as bytes [N,H,W,C]: float32 [N,C,H,W] (numpy or torch) quantised as tdr_planes_to_img_u8 does, uint8 [N,H,W,C] as it is"""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if x.dtype == np.uint8:
        return x
    assert x.dtype == np.float32 and x.ndim == 4
    q = np.rint(np.minimum(np.maximum(x, np.float32(0)), np.float32(1)) * np.float32(255.0)).astype(np.uint8)   # float32 product, ties to even
    q = q.transpose(0, 2, 3, 1)
    if swap_rb and q.shape[3] == 3:
        q = q[..., ::-1]
    return np.ascontiguousarray(q)


def crop(img, c):
    return img[:, c:img.shape[1] - c, c:img.shape[2] - c] if c else img


def y_plane(u8):
    """bytes [..., C] -> the float32 Y plane [...] of metrics.to_y_channel, operation by operation"""
    f = LUT[u8]
    if u8.shape[-1] == 1:
        return f[..., 0] * np.float32(255.)
    d = f.astype(np.float64)
    y = (((d[..., 0] * 24.966 + d[..., 1] * 128.553) + d[..., 2] * 65.481) + 16.0) / 255.0
    return y.astype(np.float32) * np.float32(255.)


def rows(pred, gt, crop_border=0, swap_rb=True, what=(), want_y=False):
    """kernels.val_metrics' rows, float64 [N, 8], with the SSIM columns left at 0 (they are the kernels' own)"""
    a, b = crop(quantise(pred, swap_rb), crop_border), crop(quantise(gt, swap_rb), crop_border)
    N = a.shape[0]
    out = np.zeros((N, 8), np.float64)
    ya, yb = y_plane(a), y_plane(b)
    for n in range(N):
        d = a[n].astype(np.int64) - b[n].astype(np.int64)
        out[n, COLS['S']], out[n, COLS['MAX']], out[n, COLS['COUNT']] = int((d * d).sum()), int(a[n].max()), d.size
        e = ya[n].astype(np.float64) - yb[n].astype(np.float64)
        out[n, COLS['SY']], out[n, COLS['COUNT_Y']] = (e * e).sum(), e.size
    return (out, ya, yb) if want_y else out


def ssim3d_f64(img1, img2, max_value):
    """the 11^3-window SSIM over the [H,W,C] volume (replicate borders) in float64 throughout, separable: the yardstick where the float32
    evaluation of oracle.metrics_oracle.ssim_3d loses the variances of a smooth image under its squared means"""
    x = np.arange(11, dtype=np.float64) - 5.0
    g = np.exp(-(x * x) / (2.0 * 1.5 * 1.5))
    g /= g.sum()

    def filt(v):
        for ax in range(3):
            p = np.pad(v, [(5, 5) if i == ax else (0, 0) for i in range(3)], mode='edge')
            v = sum(g[k] * np.take(p, range(k, k + v.shape[ax]), axis=ax) for k in range(11))
        return v
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    c1, c2 = (0.01 * max_value) ** 2, (0.03 * max_value) ** 2
    mu1, mu2 = filt(a), filt(b)
    s1, s2, s12 = filt(a * a) - mu1 * mu1, filt(b * b) - mu2 * mu2, filt(a * b) - mu1 * mu2
    return float((((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean())
