"""Generate golden vectors for the no-reference NIQE metric by running the REFERENCE (metrics/niqe.py) on the CPU.

Run in the build container only:   python tests/golden/make_golden_niqe.py [path of the reference checkout]
Writes tests/golden/niqe.npz (arrays only).

The reference module imports cv2, which is absent here; a stub module with the two calls it uses is registered first:
  * cv2.resize(img, (w // 2, h // 2), interpolation=INTER_LINEAR) -- only the exact-half case (asserted: even sizes, target = half):
    the bilinear weights are 0.5 / 0.5, evaluated like OpenCV's float path along x then along y (a * 0.5 + b * 0.5, all float32);
  * cv2.cvtColor(img, COLOR_BGR2GRAY) of a float32 image: 0.114 B + 0.587 G + 0.299 R in float32.
scipy.ndimage.filters.convolve and scipy.special.gamma import in this interpreter (scipy 1.15), so NO scipy stub was needed.
`metrics` and `utils` are entered as bare namespace packages so that metrics/__init__.py (which pulls in psnr_ssim and more third-party
imports) does not run; estimate_aggd_param, compute_feature, niqe and calculate_niqe then run UNEDITED.  calculate_niqe reads its
pristine parameters from the relative path basicsr/metrics/niqe_pris_params.npz: the script writes them there under a temporary
working directory.

Cases (every input at most 200 x 296):
  a      textured float32 Y image, 192 x 288 (2 x 3 blocks of 96), niqe() directly
  b_*    BGR uint8 image 200 x 296, crop_border 4; HWC and its CHW transpose, convert_to 'y' and 'gray'
  c      uint8 'HW' image 110 x 205: niqe() crops it to 96 x 192 (:104-107)
  d      image a with block (1, 1) AND a 6-pixel margin around it set to 128: the 7 x 7 window (3 pixels, 6 at full resolution for the
         half-size scale) then sees only the constant inside the block, its normalised map is all zero at both scales, both sides
         of every AGGD fit are empty, the betas and the Eq. 8 means are NaN (alpha is gam[0]: np.argmin of an all-NaN array is 0)
         and the row drops out of the covariance; 5 complete rows remain.
Per case: feat_ref (reference as is: float32 maps, float32 products), feat_f64 (the same functions fed the float64 copy of every
float32 block -- their dtype follows the input), score_ref, score_f64.  The normalised maps of both scales are stored for a and c in
full and for d as the patch that differs from a (asserted) -- b's maps would push the file over the 1 MiB limit for committed files;
b is pinned through its features and scores.
The reference's own float32-vs-float64 spread goes in as well: floor[36] = max over all cases of |feat_ref - feat_f64| per column, and
alpha_flip_share, the share of alpha entries where the two pick different grid points (asserted: at most 2 %, never more than one
grid step)."""
import importlib
import os
import sys
import tempfile
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
ALPHA_COLS = [0, 2, 6, 10, 14, 18, 20, 24, 28, 32]
GRID = 0.001


def cv2_stub():
    cv2 = types.ModuleType('cv2')
    cv2.INTER_LINEAR, cv2.COLOR_BGR2GRAY = 1, 6

    def resize(img, dsize, interpolation=None):
        h, w = img.shape
        assert interpolation == cv2.INTER_LINEAR and img.dtype == np.float32
        assert h % 2 == 0 and w % 2 == 0 and tuple(dsize) == (w // 2, h // 2), 'only the exact half is provided'
        half = np.float32(0.5)
        hx = img[:, 0::2] * half + img[:, 1::2] * half
        return hx[0::2] * half + hx[1::2] * half

    def cvtColor(img, code):
        assert code == cv2.COLOR_BGR2GRAY and img.dtype == np.float32 and img.ndim == 3 and img.shape[2] == 3
        return img[..., 0] * np.float32(0.114) + img[..., 1] * np.float32(0.587) + img[..., 2] * np.float32(0.299)
    cv2.resize, cv2.cvtColor = resize, cvtColor
    return cv2


def import_reference():
    sys.modules['cv2'] = cv2_stub()
    sys.path.insert(0, REF)
    for name in ('metrics', 'utils'):
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, name)]
        sys.modules[name] = m
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', DeprecationWarning)          # scipy.ndimage.filters is a deprecated alias
        return importlib.import_module('metrics.niqe')


class Recorder:
    """Stands in for the module-level name `compute_feature` while the reference's niqe() runs: records every block it is handed
    and what the reference's own compute_feature returns for it (optionally for the float64 copy of the block)."""

    def __init__(self, ref, as_f64):
        self.ref, self.orig, self.as_f64 = ref, ref.compute_feature, as_f64
        self.blocks, self.feats = [], []

    def __call__(self, block):
        self.blocks.append(np.array(block))
        f = self.orig(block.astype(np.float64) if self.as_f64 else block)
        self.feats.append(f)
        return f

    def __enter__(self):
        self.ref.compute_feature = self
        return self

    def __exit__(self, *exc):
        self.ref.compute_feature = self.orig

    def table(self):
        n = len(self.feats) // 2
        return np.concatenate([np.array(self.feats[:n], dtype=np.float64), np.array(self.feats[n:], dtype=np.float64)], axis=1)

    def maps(self, nbh, nbw):
        """the two normalised maps, reassembled from the blocks (outer loop over block columns, inner over block rows)"""
        n = nbh * nbw
        out = []
        for blocks in (self.blocks[:n], self.blocks[n:]):
            cols = [np.concatenate(blocks[c * nbh:(c + 1) * nbh], axis=0) for c in range(nbw)]
            out.append(np.concatenate(cols, axis=1))
        return out


def run(ref, fn):
    """fn() calls into the reference; -> (score_ref, feat_ref, score_f64, feat_f64, blocks)"""
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')                  # 'Mean of empty slice' of case d
        with Recorder(ref, False) as r32:
            s32 = float(np.squeeze(fn()))
        with Recorder(ref, True) as r64:
            s64 = float(np.squeeze(fn()))
    assert all(b.dtype == np.float32 for b in r32.blocks)
    assert all(np.array_equal(a, b) for a, b in zip(r32.blocks, r64.blocks))
    return s32, r32.table(), s64, r64.table(), r32


def textured(rng, h, w, smooth=1.0, noise=18.0):
    from scipy import ndimage
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 120 + 45 * np.sin(yy / 9.0 + 0.3) * np.cos(xx / 13.0) + 25 * np.sin((xx + 2 * yy) / 31.0)
    tex = ndimage.gaussian_filter(rng.normal(0, noise, (h, w)), smooth) * (1.0 + 0.8 * np.sin(yy / 37.0) * np.sin(xx / 29.0))
    return np.clip(base + tex + rng.normal(0, 2.0, (h, w)), 0, 255)


def gaussian_window():
    """fspecial('gaussian', 7, 7 / 6)"""
    x = np.arange(7, dtype=np.float64) - 3
    g = np.exp(-(x[:, None] ** 2 + x[None, :] ** 2) / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def main():
    ref = import_reference()
    d = {}
    window = gaussian_window()

    # pristine model: the reference's features of a few smooth seeded images
    rows = []
    for seed in range(8):
        img = textured(np.random.default_rng(100 + seed), 192, 288, smooth=1.6 + 0.2 * seed, noise=30.0).astype(np.float32)
        _, _, _, f64, _ = run(ref, lambda: ref.niqe(img, np.zeros((1, 36)), np.eye(36), window))
        rows.append(f64)
    rows = np.concatenate(rows, axis=0)
    assert np.isfinite(rows).all() and rows.shape[0] > 36
    mu = rows.mean(axis=0, keepdims=True)
    cov = np.cov(rows, rowvar=False)
    d['mu_pris_param'], d['cov_pris_param'], d['gaussian_window'] = mu, cov, window
    print('pristine model from', rows.shape[0], 'blocks; cond(cov) = %.3g' % np.linalg.cond(cov))

    rng = np.random.default_rng(7)
    a = textured(rng, 192, 288).astype(np.float32)
    b = np.clip(np.stack([textured(rng, 200, 296, smooth=0.8 + 0.3 * c) for c in range(3)], axis=-1).round(), 0, 255).astype(np.uint8)
    c_img = np.clip(textured(rng, 110, 205).round(), 0, 255).astype(np.uint8)
    region = np.array([96 - 6, 192, 96 - 6, 192 + 6])            # block (1, 1) of the 2 x 3 grid + the margin (the image ends at row 192)
    d_img = a.copy()
    d_img[region[0]:region[1], region[2]:region[3]] = 128.0
    d['a_img'], d['b_img'], d['c_img'], d['d_region'], d['d_value'] = a, b, c_img, region, np.float32(128.0)
    d['b_crop_border'] = np.array(4)

    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, 'basicsr', 'metrics'))
        np.savez(os.path.join(tmp, 'basicsr', 'metrics', 'niqe_pris_params.npz'), mu_pris_param=mu, cov_pris_param=cov,
                 gaussian_window=window)
        os.chdir(tmp)
        try:
            cases = {
                'a': lambda: ref.niqe(a, mu, cov, window),
                'b_hwc_y': lambda: ref.calculate_niqe(b, 4, input_order='HWC', convert_to='y'),
                'b_chw_y': lambda: ref.calculate_niqe(np.ascontiguousarray(b.transpose(2, 0, 1)), 4, input_order='CHW', convert_to='y'),
                'b_hwc_gray': lambda: ref.calculate_niqe(b, 4, input_order='HWC', convert_to='gray'),
                'b_chw_gray': lambda: ref.calculate_niqe(np.ascontiguousarray(b.transpose(2, 0, 1)), 4, input_order='CHW', convert_to='gray'),
                'c': lambda: ref.calculate_niqe(c_img, 0, input_order='HW'),
                'd': lambda: ref.niqe(d_img, mu, cov, window),
            }
            res = {k: run(ref, fn) for k, fn in cases.items()}
        finally:
            os.chdir(cwd)

    floor = np.zeros(36)
    flips = total = 0
    for k, (s32, f32, s64, f64, rec) in res.items():
        assert np.array_equal(np.isnan(f32), np.isnan(f64))
        assert np.isfinite(s32) and np.isfinite(s64) and s64 > 0
        d[f'{k}_feat_ref'], d[f'{k}_feat_f64'], d[f'{k}_score_ref'], d[f'{k}_score_f64'] = f32, f64, np.array(s32), np.array(s64)
        diff = np.abs(f32 - f64)
        floor = np.fmax(floor, np.nanmax(diff, axis=0))
        da = diff[:, ALPHA_COLS]
        assert np.nanmax(da) <= GRID * 1.5, 'the reference itself moves an alpha by more than one grid step'
        flips += int((da > GRID / 2).sum())
        total += da.size
        print(f'{k:11s} blocks {f64.shape[0]}  score_ref {s32:.9f}  score_f64 {s64:.9f}  rel {abs(s32 - s64) / s64:.2e}  '
              f'nan rows {int(np.isnan(f64).any(axis=1).sum())}')
    for k in ('b_chw_y', 'b_chw_gray'):
        assert np.array_equal(d[f'{k}_feat_ref'], d[k.replace('chw', 'hwc') + '_feat_ref'], equal_nan=True)
    share = flips / total
    assert share <= 0.02, f'alpha flip share {share}: choose other seeds'
    d['floor'], d['alpha_flip_share'] = floor, np.array(share)
    print('alpha flips', flips, 'of', total, '; floor of the non-alpha columns: max %.3g' % np.delete(floor, ALPHA_COLS).max())

    nanrows = np.isnan(d['d_feat_f64']).any(axis=1)
    assert nanrows.sum() == 1 and nanrows[1 * 2 + 1] and (~nanrows).sum() >= 4          # block (1, 1): index idx_w * nbh + idx_h
    assert np.array_equal(d['d_feat_f64'][3, ALPHA_COLS], np.full(10, 0.2))             # alpha = gam[argmin(all NaN)] = gam[0]
    assert np.isnan(np.delete(d['d_feat_f64'][3], ALPHA_COLS)).all()

    a1, a2 = res['a'][4].maps(2, 3)
    c1, c2 = res['c'][4].maps(1, 2)
    d1, d2 = res['d'][4].maps(2, 3)
    patch = np.array([region[0] - 6, 192, region[2] - 6, region[3] + 6])                # what the change can reach: 3 pixels, 6 for the half scale
    m1, m2 = np.ones_like(a1, dtype=bool), np.ones_like(a2, dtype=bool)
    m1[patch[0]:patch[1], patch[2]:patch[3]] = False
    m2[patch[0] // 2:patch[1] // 2, patch[2] // 2:patch[3] // 2] = False
    assert np.array_equal(a1[m1], d1[m1]) and np.array_equal(a2[m2], d2[m2])
    assert not d1[96:192, 96:192].any() and not d2[48:96, 48:96].any()
    d['a_map1'], d['a_map2'], d['c_map1'], d['c_map2'] = a1, a2, c1, c2
    d['d_patch'] = patch
    d['d_map1_patch'] = d1[patch[0]:patch[1], patch[2]:patch[3]]
    d['d_map2_patch'] = d2[patch[0] // 2:patch[1] // 2, patch[2] // 2:patch[3] // 2]

    gam = np.arange(0.2, 10.001, 0.001)
    from scipy.special import gamma
    d['gam'] = gam
    rec = np.reciprocal(gam)
    d['r_gam'] = np.square(gamma(rec * 2)) / (gamma(rec) * gamma(rec * 3))               # the expression of :21-24
    out = os.path.join(HERE, 'niqe.npz')
    np.savez_compressed(out, **d)
    print('wrote niqe.npz', len(d), 'arrays', os.path.getsize(out), 'bytes')


if __name__ == '__main__':
    main()
