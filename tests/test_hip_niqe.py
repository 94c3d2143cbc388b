"""NIQE on the device (csrc/tdr_niqe.hip) against the REFERENCE's metrics/niqe.py run on the CPU (tests/golden/make_golden_niqe.py).

Every bar comes from the golden file, never from the code under test: `floor[c]` is the reference's own float32-vs-float64 spread of
feature column c (the same reference functions fed the float32 blocks and their float64 copies), `alpha_flip_share` the share of
alpha entries where those two pick different grid points, score_ref / score_f64 the two resulting scores.  The device computes
float64 moments over the float32 maps, i.e. it sits on the float64 side; the floor is doubled because it departs from the
reference's float32 run on the other side."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'niqe.npz')
ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
OTHER_COLS = [c for c in range(36) if c not in ALPHA_COLS]
GRID = 0.001
PRIS = ('mu_pris_param', 'cov_pris_param', 'gaussian_window')

pytestmark = pytest.mark.gpu


def need_gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')


def y_of(g, case):
    """the [h, w] float32 image the reference hands to niqe() for a golden case, whole blocks only"""
    from textualdegremoval_amd.metrics import to_y_channel
    if case == 'a':
        return g['a_img']
    if case == 'd':
        img = g['a_img'].copy()
        r = g['d_region']
        img[r[0]:r[1], r[2]:r[3]] = g['d_value']
        return img
    if case == 'c':
        img = g['c_img'].astype(np.float32)
        return img[:img.shape[0] // 96 * 96, :img.shape[1] // 96 * 96]
    img = g['b_img'].astype(np.float32)
    if case.endswith('_y'):
        img = np.squeeze(to_y_channel(img))
    else:
        img = img / 255.
        img = (img[..., 0] * np.float32(0.114) + img[..., 1] * np.float32(0.587) + img[..., 2] * np.float32(0.299)) * 255.
    cb = int(g['b_crop_border'])
    return np.ascontiguousarray(img[cb:-cb, cb:-cb])


def device_features(g, case, maps=False):
    from textualdegremoval_amd import kernels as K
    y = torch.from_numpy(np.ascontiguousarray(y_of(g, case), dtype=np.float32)).cuda()
    return K.niqe_features(y, g['gaussian_window'], 96, return_maps=maps)


def golden_maps(g, case):
    if case != 'd':
        return g[f'{case}_map1'], g[f'{case}_map2']
    m1, m2, p = g['a_map1'].copy(), g['a_map2'].copy(), g['d_patch']
    m1[p[0]:p[1], p[2]:p[3]] = g['d_map1_patch']
    m2[p[0] // 2:p[1] // 2, p[2] // 2:p[3] // 2] = g['d_map2_patch']
    return m1, m2


@pytest.mark.parametrize('case', ['a', 'c', 'd'])
def test_normalised_maps_of_both_scales(case):
    """the only freedom is the order of a 49-term double sum ahead of one float32 rounding: 2 float32 ulp of the map's maximum"""
    need_gpu()
    g = np.load(GOLDEN)
    _, n1, n2 = device_features(g, case, maps=True)
    for scale, (got, want) in enumerate(zip((n1, n2), golden_maps(g, case)), 1):
        got = got.cpu().numpy()
        assert got.shape == want.shape and got.dtype == np.float32
        bar = 2 * float(np.spacing(np.float32(np.abs(want).max())))
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        print(f'{case} scale {scale}: max |dev - ref| {err:.3e} (bar {bar:.3e}), exact in {float((got == want).mean()):.6f} of the pixels')
        assert err <= bar, (case, scale, err, bar)
    if case == 'd':
        assert not n1[96:192, 96:192].any() and not n2[48:96, 48:96].any()          # the constant block: exactly zero


@pytest.mark.parametrize('case', ['a', 'b_hwc_y', 'b_hwc_gray', 'c', 'd'])
def test_features_against_the_float64_reference(case):
    need_gpu()
    g = np.load(GOLDEN)
    dev = device_features(g, case).cpu().numpy()
    f64, floor = g[f'{case}_feat_f64'], g['floor']
    assert dev.shape == f64.shape and dev.dtype == np.float64
    assert np.array_equal(np.isnan(dev), np.isnan(f64))
    for c in OTHER_COLS:
        bar = 2 * floor[c] + 1e-9 * np.nanmax(np.abs(f64[:, c]))
        err = np.nanmax(np.abs(dev[:, c] - f64[:, c]))
        print(f'{case} column {c}: max |dev - f64| {err:.3e} (bar {bar:.3e})')
        assert err <= bar, (case, c, err, bar)
    da = np.abs(dev[:, ALPHA_COLS] - f64[:, ALPHA_COLS])
    moved = da != 0
    print(f'{case} alpha entries moved: {int(moved.sum())} of {moved.size}')
    assert moved.mean() <= max(float(g['alpha_flip_share']), 0.02)
    assert np.all(np.abs(da[moved] - GRID) <= 1e-12)                                 # each of them by exactly one grid step


@pytest.mark.parametrize('case,kw', [
    ('a', None), ('d', None),
    ('b_hwc_y', dict(crop_border=4, input_order='HWC', convert_to='y')), ('b_chw_y', dict(crop_border=4, input_order='CHW', convert_to='y')),
    ('b_hwc_gray', dict(crop_border=4, input_order='HWC', convert_to='gray')),
    ('b_chw_gray', dict(crop_border=4, input_order='CHW', convert_to='gray')),
    ('c', dict(crop_border=0, input_order='HW'))])
def test_scores_end_to_end(case, kw):
    need_gpu()
    from textualdegremoval_amd.metrics import calculate_niqe, niqe
    g = np.load(GOLDEN)
    pris = {k: g[k] for k in PRIS}
    if kw is None:                                           # the cases the golden script ran through niqe() directly
        got = niqe(y_of(g, case), *[g[k] for k in PRIS])
    else:
        img = g['c_img'] if case == 'c' else g['b_img']
        if kw['input_order'] == 'CHW':
            img = np.ascontiguousarray(img.transpose(2, 0, 1))
        got = calculate_niqe(img, kw['crop_border'], kw['input_order'], kw.get('convert_to', 'y'), pris_params=pris)
    got = float(np.squeeze(got))
    ref, f64 = float(g[f'{case}_score_ref']), float(g[f'{case}_score_f64'])
    bar = 4 * abs(ref - f64) / f64 + 1e-6
    print(f'{case}: device {got:.9f} f64 {f64:.9f} ref {ref:.9f} rel {abs(got - f64) / f64:.3e} (bar {bar:.3e})')
    assert np.isfinite(got) and got > 0
    assert abs(got - f64) / f64 <= bar, (case, got, f64, bar)


def test_params_file_path_and_default_location(tmp_path, monkeypatch):
    """pris_params as a path, and the reference's relative default resolved against the working directory"""
    need_gpu()
    from textualdegremoval_amd.metrics import calculate_niqe
    g = np.load(GOLDEN)
    os.makedirs(tmp_path / 'basicsr' / 'metrics')
    path = tmp_path / 'basicsr' / 'metrics' / 'niqe_pris_params.npz'
    np.savez(path, **{k: g[k] for k in PRIS})
    want = float(np.squeeze(calculate_niqe(g['b_img'], 4, pris_params={k: g[k] for k in PRIS})))
    assert float(np.squeeze(calculate_niqe(g['b_img'], 4, pris_params=str(path)))) == want
    monkeypatch.chdir(tmp_path)
    assert float(np.squeeze(calculate_niqe(g['b_img'], 4))) == want


def test_two_calls_are_bit_identical():
    need_gpu()
    g = np.load(GOLDEN)
    for case in ('a', 'd'):
        f1 = device_features(g, case).cpu().numpy()
        f2 = device_features(g, case).cpu().numpy()
        assert f1.tobytes() == f2.tobytes()


def test_device_tensor_and_ndarray_agree():
    need_gpu()
    from textualdegremoval_amd.metrics import calculate_niqe, niqe
    g = np.load(GOLDEN)
    pris = [g[k] for k in PRIS]
    a = niqe(g['a_img'], *pris)
    b = niqe(torch.from_numpy(g['a_img']).cuda(), *pris)
    assert float(np.squeeze(a)) == float(np.squeeze(b))
    c = calculate_niqe(g['b_img'], 4, pris_params=dict(zip(PRIS, pris)))
    d = calculate_niqe(torch.from_numpy(g['b_img']).cuda(), 4, pris_params=dict(zip(PRIS, pris)))
    assert float(np.squeeze(c)) == float(np.squeeze(d))


def test_bad_geometry_is_an_error_not_a_launch():
    need_gpu()
    from textualdegremoval_amd import _lib, kernels as K
    g = np.load(GOLDEN)
    y = torch.zeros(100, 192, device='cuda')
    with pytest.raises(_lib.TdrError, match='whole number'):
        K.niqe_features(y, g['gaussian_window'], 96)
