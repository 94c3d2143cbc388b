"""PSNR / SSIM of `use_image: true` validation from device tensors (csrc/tdr_valmetrics.hip): the restored image and its ground truth are
quantised, cropped, compared and reduced where they are, and the numbers are read back once per validation instead of three images per
validated image.  The image domain is bytes, so the device path is held to the bits of the host path (tensor2img, then calculate_psnr /
calculate_ssim of this package): the squared error is an integer, the SSIM kernels share their arithmetic with K.ssim3d / K.ssim_y64."""
import numpy as np
import torch

_TYPES = ('calculate_psnr', 'calculate_ssim')
_U255 = np.float32(255.)


def _psnr_finish(row, y, channels):
    """calculate_psnr's tail in float64 numpy, from one row of kernels.val_metrics"""
    from .. import kernels as K
    s, count = (row[K.VALM_SY], row[K.VALM_COUNT_Y]) if y else (row[K.VALM_S], row[K.VALM_COUNT])
    mse = np.float64(s) / np.float64(count)
    if mse == 0:
        return float('inf')
    top = row[K.VALM_MAX]
    if y:
        # the largest Y: >= 16 for a colour image; for a gray one float32(u) / 255 * 255 of the largest byte (monotonic in u)
        top = 255. if channels == 3 else np.float32(np.float32(top) / _U255) * _U255
    max_value = 1. if top <= 1 else 255.
    return 20. * np.log10(max_value / np.sqrt(mse))


class ValMetrics:
    """The metrics of one validation, accumulated on the device.  spec: a `val.metrics` option block,
    {name: {type: calculate_psnr | calculate_ssim, crop_border, test_y_channel, input_order?}}."""

    def __init__(self, spec, use_image=True, kernel=None):
        from .. import kernels as K
        if not use_image:
            raise ValueError('device metrics are defined on the byte images of `use_image: true` (tensor2img, then the metric); the float '
                             'domain of `use_image: false` has no exact sum to hold them to')
        if not spec:
            raise ValueError('ValMetrics: an empty val.metrics block')
        self.entries = []                       # (name, column kind, crop)
        self._calls = {}                        # crop -> set of `what`
        for name, opt in spec.items():
            opt = dict(opt)
            kind = opt.pop('type', None)
            if kind not in _TYPES:
                raise ValueError(f'val.metrics.{name}: type {kind!r} has no device path (val.device_metrics supports {", ".join(_TYPES)})')
            order = opt.pop('input_order', 'HWC')
            if order not in ('HWC', 'CHW'):
                raise ValueError(f'Wrong input_order {order}. Supported input_orders are "HWC" and "CHW"')
            crop, y = int(opt.pop('crop_border', 0)), bool(opt.pop('test_y_channel', False))
            if opt:
                raise ValueError(f'val.metrics.{name}: unknown option(s) {sorted(opt)}')
            what = ('psnr' if kind == 'calculate_psnr' else 'ssim') + ('_y' if y else '')
            self.entries.append((name, what, crop))
            self._calls.setdefault(crop, set()).add(what)
        self._order = ('psnr', 'ssim', 'psnr_y', 'ssim_y')
        self._kernel = kernel or K.val_metrics  # (`kernel`: a stand-in with val_metrics' signature and rows, for tests without a GPU)
        self._rows = {crop: [] for crop in self._calls}
        self._channels = None
        self.per_image = {}

    def add(self, pred, gt, rgb2bgr=True):
        """pred / gt: device tensors, float32 [N,C,H,W] or uint8 [N,H,W,C].  One kernels.val_metrics call per distinct crop_border covers
        every metric of the spec; the rows stay on the device, nothing is synchronised."""
        channels = pred.shape[3] if pred.dtype == torch.uint8 else pred.shape[1]
        if self._channels not in (None, channels):
            raise ValueError(f'ValMetrics.add: {channels} channels after {self._channels}')
        self._channels = channels
        for crop, what in self._calls.items():
            self._rows[crop].append(self._kernel(pred, gt, crop_border=crop, swap_rb=rgb2bgr,
                                                 what=tuple(w for w in self._order if w in what)))

    def result(self):
        """One copy of all rows to the host, then per image and metric the float64 finish of calculate_psnr -> {name: mean}, the means
        summed in arrival order and divided as the validation loop does.  `.per_image` keeps {name: [value per image]}."""
        from .. import kernels as K
        crops = sorted(self._rows)
        count = sum(r.shape[0] for r in self._rows[crops[0]]) if crops else 0
        if count == 0:
            self.per_image = {name: [] for name, _, _ in self.entries}
            return {name: 0 for name, _, _ in self.entries}
        rows = torch.cat([r for crop in crops for r in self._rows[crop]]).cpu().numpy()          # the one synchronising copy
        rows = {crop: rows[i * count:(i + 1) * count] for i, crop in enumerate(crops)}
        self.per_image, means = {}, {}
        for name, what, crop in self.entries:
            if what.startswith('psnr'):
                vals = [_psnr_finish(r, what == 'psnr_y', self._channels) for r in rows[crop]]
            else:
                vals = [float(r[K.VALM_SSIMY if what == 'ssim_y' else K.VALM_SSIM3D]) for r in rows[crop]]
            total = 0
            for v in vals:
                total += v
            self.per_image[name], means[name] = vals, total / max(count, 1)
        return means


def psnr_ssim(pred, gt, crop_border=0, test_y_channel=False, rgb2bgr=True):
    """(PSNR, SSIM) of device tensors as calculate_psnr / calculate_ssim give them for tensor2img(pred, rgb2bgr) and tensor2img(gt, rgb2bgr);
    the mean over the images of a batch.  Synchronises once."""
    opt = {'crop_border': crop_border, 'test_y_channel': test_y_channel}
    vm = ValMetrics({'psnr': dict(opt, type='calculate_psnr'), 'ssim': dict(opt, type='calculate_ssim')})
    vm.add(pred, gt, rgb2bgr)
    res = vm.result()
    return res['psnr'], res['ssim']
