"""NIQE, the no-reference quality metric, with the reference's semantics (metrics/niqe.py): the normalised maps of two scales and
the 18 AGGD features per 96 x 96 block and scale come from the device (csrc/tdr_niqe.hip through kernels.niqe_features; there is
no host fallback), the multivariate-Gaussian tail over the [nblocks, 36] table runs on the host in float64 as the reference's does."""
import math
import os

import numpy as np
import torch

from . import to_y_channel

# calculate_niqe of the reference loads this relative path (:186); the file is not part of the reference tree
DEFAULT_PRIS_PARAMS = 'basicsr/metrics/niqe_pris_params.npz'
_PRIS_KEYS = ('mu_pris_param', 'cov_pris_param', 'gaussian_window')


def reorder_image(img, input_order='HWC'):
    """(h, w) -> (h, w, 1); (c, h, w) -> (h, w, c); (h, w, c) as it is (metrics/metric_util.py:6-31)"""
    if input_order not in ['HWC', 'CHW']:
        raise ValueError(f'Wrong input_order {input_order}. Supported input_orders are ' "'HWC' and 'CHW'")
    if len(img.shape) == 2:
        img = img[..., None]
    if input_order == 'CHW':
        img = img.transpose(1, 2, 0)
    return img


def niqe_from_features(feats, mu_pris_param, cov_pris_param):
    """The tail of niqe (:140-155): feats float64 [nblocks, 36] -> sqrt((mu_p - mu_d) pinv((cov_p + cov_d) / 2) (mu_p - mu_d)^T), with
    nanmean over the rows and the covariance of the rows without NaN.  The result has the shape the reference's has ([1, 1] for a
    [1, 36] mu_pris_param)."""
    distparam = np.asarray(feats, dtype=np.float64)
    mu_distparam = np.nanmean(distparam, axis=0)
    distparam_no_nan = distparam[~np.isnan(distparam).any(axis=1)]
    cov_distparam = np.cov(distparam_no_nan, rowvar=False)
    invcov_param = np.linalg.pinv((cov_pris_param + cov_distparam) / 2)
    quality = np.matmul(np.matmul((mu_pris_param - mu_distparam), invcov_param), np.transpose((mu_pris_param - mu_distparam)))
    return np.sqrt(quality)


def niqe(img, mu_pris_param, cov_pris_param, gaussian_window, block_size_h=96, block_size_w=96):
    """niqe of the reference (:67-155).  img: ndarray or tensor [h, w], gray or Y in [0, 255]; it is taken as float32, the format
    calculate_niqe hands over.  Blocks are square with an even side on the HIP path."""
    from .. import kernels as K
    assert img.ndim == 2, ('Input image must be a gray or Y (of YCbCr) image with shape (h, w).')
    if block_size_h != block_size_w or block_size_h % 2 != 0 or block_size_h <= 0:
        raise NotImplementedError(f'niqe: the HIP path handles square blocks with an even side, got {block_size_h} x {block_size_w}')
    if not torch.cuda.is_available():
        raise RuntimeError('niqe: the HIP path needs tensors on the MI355X; there is no CPU fallback')
    h, w = img.shape
    num_block_h = math.floor(h / block_size_h)
    num_block_w = math.floor(w / block_size_w)
    if not isinstance(img, torch.Tensor):
        img = torch.from_numpy(np.ascontiguousarray(img, dtype=np.float32))
    if not img.is_cuda:
        img = img.to(torch.device('cuda', torch.cuda.current_device()))
    img = img.detach()[0:num_block_h * block_size_h, 0:num_block_w * block_size_w].float().contiguous()
    feats = K.niqe_features(img, gaussian_window, block_size_h)
    return niqe_from_features(feats.cpu().numpy(), mu_pris_param, cov_pris_param)


def _load_pris_params(pris_params):
    if pris_params is None:
        pris_params = DEFAULT_PRIS_PARAMS
    if isinstance(pris_params, (str, os.PathLike)):
        if not os.path.exists(pris_params):
            raise FileNotFoundError(f'calculate_niqe: no pristine-model parameters at {os.fspath(pris_params)!r}; pass pris_params= (a path '
                                    f'to an .npz or a mapping with {", ".join(_PRIS_KEYS)})')
        pris_params = np.load(pris_params)
    return tuple(np.asarray(pris_params[k]) for k in _PRIS_KEYS)


def calculate_niqe(img, crop_border, input_order='HWC', convert_to='y', pris_params=None):
    """calculate_niqe of the reference (:158-205): img in [0, 255], 'HW', 'HWC' or 'CHW' (BGR); 'HWC' / 'CHW' images are converted to
    Y of BT.601 YCbCr ('y') or to gray.  pris_params: a path to the .npz with mu_pris_param [1, 36], cov_pris_param [36, 36] and
    gaussian_window [7, 7], or a mapping with those keys; None is the reference's relative path."""
    mu_pris_param, cov_pris_param, gaussian_window = _load_pris_params(pris_params)
    if isinstance(img, torch.Tensor):
        img = img.detach().cpu().numpy()
    img = img.astype(np.float32)
    if input_order != 'HW':
        img = reorder_image(img, input_order=input_order)
        if convert_to == 'y':
            img = to_y_channel(img)
        elif convert_to == 'gray':
            # cv2.cvtColor(img / 255., cv2.COLOR_BGR2GRAY) * 255. of a float32 BGR image
            img = img / 255.
            img = (img[..., 0] * np.float32(0.114) + img[..., 1] * np.float32(0.587) + img[..., 2] * np.float32(0.299)) * 255.
        img = np.squeeze(img)
    if crop_border != 0:
        img = img[crop_border:-crop_border, crop_border:-crop_border]
    return niqe(img, mu_pris_param, cov_pris_param, gaussian_window)
