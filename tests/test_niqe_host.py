"""NIQE, the parts that need no GPU: the public names, the float64 Gaussian-model tail against the scores the REFERENCE computed
(tests/golden/make_golden_niqe.py runs metrics/niqe.py on the CPU), the host gamma tables, argument errors and the C-ABI declarations."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'niqe.npz')
CASES = ['a', 'b_hwc_y', 'b_chw_y', 'b_hwc_gray', 'b_chw_gray', 'c', 'd']


def test_public_names():
    import textualdegremoval_amd.metrics as M
    for name in ('calculate_psnr', 'calculate_ssim', 'calculate_niqe', 'niqe', 'niqe_from_features', 'tensor2img', 'to_y_channel',
                 'bgr2ycbcr_y'):
        assert callable(getattr(M, name)), name


@pytest.mark.parametrize('case', CASES)
def test_tail_matches_the_reference_scores(case):
    """same float64 LAPACK tail on both sides; case d carries the NaN row that nanmean keeps out of the mean and the covariance drops"""
    from textualdegremoval_amd.metrics import niqe_from_features
    g = np.load(GOLDEN)
    mu, cov = g['mu_pris_param'], g['cov_pris_param']
    for which in ('f64', 'ref'):
        want = float(g[f'{case}_score_{which}'])
        got = niqe_from_features(g[f'{case}_feat_{which}'], mu, cov)
        assert got.shape == (1, 1)                          # what the reference returns for a [1, 36] mu_pris_param
        assert abs(float(got[0, 0]) - want) <= 1e-9 * want, (case, which, float(got[0, 0]), want)
    if case == 'd':
        nan_rows = np.isnan(g['d_feat_f64']).any(axis=1)
        assert nan_rows.sum() == 1 and (~nan_rows).sum() >= 4


def test_host_gamma_tables_match_the_reference_table():
    from textualdegremoval_amd import kernels as K
    from math import gamma
    g = np.load(GOLDEN)
    tab = K.niqe_gamma_tables()
    assert tab.shape == (4, 9801) and tab.dtype == np.float64
    assert np.array_equal(tab[0], g['gam'])                 # the grid itself: np.arange(0.2, 10.001, 0.001), bit for bit
    assert np.abs(tab[1] / g['r_gam'] - 1).max() <= 1e-12
    for i in (0, 800, 1800, 9800):                          # alpha 0.2, 1.0, 2.0 (Gaussian: r_gam = 2 / pi), 10.0
        a = tab[0, i]
        assert abs(tab[2, i] / np.sqrt(gamma(1 / a) / gamma(3 / a)) - 1) <= 1e-14
        assert abs(tab[3, i] / (gamma(2 / a) / gamma(1 / a)) - 1) <= 1e-14
    assert abs(tab[1, 1800] - 2 / np.pi) <= 1e-14


def test_reorder_image_semantics_and_error():
    from textualdegremoval_amd.metrics.niqe import reorder_image
    x = np.zeros((3, 4, 5))
    assert reorder_image(x).shape == (3, 4, 5) and reorder_image(x, 'CHW').shape == (4, 5, 3)
    assert reorder_image(np.zeros((4, 5))).shape == (4, 5, 1)
    with pytest.raises(ValueError, match="Wrong input_order HW. Supported input_orders are 'HWC' and 'CHW'"):
        reorder_image(x, 'HW')
    from textualdegremoval_amd.metrics import calculate_niqe
    g = np.load(GOLDEN)
    with pytest.raises(ValueError, match='Wrong input_order BCHW'):
        calculate_niqe(g['b_img'], 4, input_order='BCHW', pris_params={k: g[k] for k in ('mu_pris_param', 'cov_pris_param', 'gaussian_window')})


def test_missing_params_file_names_the_path_and_the_keyword(tmp_path, monkeypatch):
    from textualdegremoval_amd.metrics import calculate_niqe
    img = np.zeros((96, 96, 3), dtype=np.uint8)
    monkeypatch.chdir(tmp_path)                             # the reference's relative default cannot exist here
    with pytest.raises(FileNotFoundError, match=r'basicsr/metrics/niqe_pris_params\.npz.*pris_params'):
        calculate_niqe(img, 0)
    with pytest.raises(FileNotFoundError, match=r'nowhere\.npz.*pris_params'):
        calculate_niqe(img, 0, pris_params=str(tmp_path / 'nowhere.npz'))
    with pytest.raises(TypeError):                          # crop_border is positional and required, as in the reference
        calculate_niqe(img)


def test_block_size_limits_and_shape_assertion():
    from textualdegremoval_amd.metrics import niqe
    g = np.load(GOLDEN)
    mu, cov, win = g['mu_pris_param'], g['cov_pris_param'], g['gaussian_window']
    with pytest.raises(NotImplementedError, match='square blocks with an even side'):
        niqe(g['a_img'], mu, cov, win, 96, 48)
    with pytest.raises(NotImplementedError, match='square blocks with an even side'):
        niqe(g['a_img'], mu, cov, win, 95, 95)
    with pytest.raises(AssertionError, match=r'Input image must be a gray or Y \(of YCbCr\) image with shape \(h, w\)\.'):
        niqe(g['b_img'], mu, cov, win)


def test_no_cpu_fallback(monkeypatch):
    from textualdegremoval_amd.metrics import niqe
    g = np.load(GOLDEN)
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        niqe(g['a_img'], g['mu_pris_param'], g['cov_pris_param'], g['gaussian_window'])


def test_abi_declares_the_niqe_entry_points():
    from textualdegremoval_amd import _lib
    txt = open(os.path.join(ROOT, 'include', 'tdr.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for name in ('tdr_niqe_ws_floats', 'tdr_niqe_features'):
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert name in _lib.SIGNATURES
    assert int(re.search(r'#define TDR_ABI_VERSION (\d+)', txt).group(1)) == _lib.ABI_VERSION >= 109
    lib = _lib.load()
    assert lib.tdr_niqe_ws_floats(192, 288) == 192 * 288 + 2 * 96 * 144
    for args in ((192, 288, 95), (192, 200, 96), (48, 96, 96)):          # odd block; W not a multiple; no whole block
        rc = lib.tdr_niqe_features(8, args[0], args[1], args[2], 8, 8, 9801, 8, 8, None)     # rejected before anything is launched
        assert rc < 0 and b'tdr_niqe_features' in lib.tdr_last_error()
