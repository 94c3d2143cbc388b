"""Device validation metrics, the parts that need no GPU: the two entry points of csrc/tdr_valmetrics.hip in the header, the binding and
the built library; the host finish of metrics.device against metrics.calculate_psnr, bit for bit; the explicit-order Y plane against
metrics.to_y_channel for every one of the 2^24 colours; ValMetrics' spec errors and its means against the sequential host loop, with the
numpy reference of tests/_val_metrics_ref.py standing in for the kernel."""
import os
import re
import struct

import numpy as np
import pytest
import torch

import _val_metrics_ref as VR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('tdr_val_metrics_ws_bytes', 'tdr_val_metrics')


def _bits(x):
    return struct.pack('<d', float(x))


def test_header_declares_the_val_metrics_entry_points():
    txt = open(os.path.join(ROOT, 'include', 'tdr.h')).read()
    head = txt[:txt.index('#define TDR_ABI_VERSION')]
    assert 'tdr_val_metrics_ws_bytes / tdr_val_metrics' in head                            # (listed among the additions to ABI 112)
    assert re.search(r'#define TDR_ABI_VERSION 112\b', txt)
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert set(NEW) <= set(re.findall(r'\b(tdr_[a-z0-9_]+)\s*\(', code))


def test_binding_and_library_have_them():
    from textualdegremoval_amd import _lib
    assert _lib.ABI_VERSION == 112
    lib = _lib.load()                                                                      # raises if a declared symbol is missing
    for s in NEW:
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['tdr_val_metrics_ws_bytes'][1]) == 3 and len(_lib.SIGNATURES['tdr_val_metrics'][1]) == 22
    assert lib.tdr_version() == 112
    assert lib.tdr_val_metrics_ws_bytes(2, 37, 53) >= 2 * 2 * 37 * 53 * 3
    # refusals come back as error codes before anything is launched
    assert lib.tdr_val_metrics(None, None, 0, 0, 0, None, None, 0, 0, 0, 1, 3, 8, 8, 0, 0, 1, None, None, None, None, None) != 0
    assert 'exactly one' in lib.tdr_last_error().decode()


def _images(rng, kind, H=37, W=53):
    C = 1 if kind == 'gray' else 3
    a = rng.integers(0, 256, (1, H, W, C), dtype=np.uint8)
    b = np.clip(a.astype(np.int64) + rng.integers(-9, 10, a.shape), 0, 255).astype(np.uint8)
    if kind == 'same':
        b = a.copy()
    if kind == 'unit':                       # every byte <= 1: max_value 1
        a, b = (a & 1).astype(np.uint8), (b & 1).astype(np.uint8)
    return a, b


@pytest.mark.parametrize('crop', [0, 4])
@pytest.mark.parametrize('kind', ['rgb', 'gray', 'same', 'unit'])
def test_host_finish_equals_calculate_psnr(kind, crop):
    from textualdegremoval_amd.metrics import calculate_psnr
    from textualdegremoval_amd.metrics.device import _psnr_finish
    a, b = _images(np.random.default_rng(7 + crop), kind)
    row = VR.rows(a, b, crop)[0]
    sq = (lambda x: x[0, :, :, 0]) if kind == 'gray' else (lambda x: x[0])               # (tensor2img hands a gray image over as [H, W])
    want = calculate_psnr(sq(a), sq(b), crop)
    got = _psnr_finish(row, False, a.shape[3])
    assert _bits(got) == _bits(want), (got, want)
    if kind == 'same':
        assert got == float('inf')
    if kind == 'unit':
        assert row[VR.COLS['MAX']] == 1 and got < 20                                    # (the unit constant: 20 log10(1 / sqrt(mse)))


@pytest.mark.parametrize('swap', [False, True])
def test_y_plane_of_all_colours(swap):
    from textualdegremoval_amd.metrics import to_y_channel
    v = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([v & 255, (v >> 8) & 255, v >> 16], -1).astype(np.uint8).reshape(4096, 4096, 3)
    if swap:                                  # the coefficients go by position: swapping the source swaps what they meet
        img = np.ascontiguousarray(img[..., ::-1])
    want = to_y_channel(img.astype(np.float64))[..., 0]
    got = VR.y_plane(img)
    assert got.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    gray = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    assert np.array_equal(VR.y_plane(gray).view(np.uint32), to_y_channel(gray.astype(np.float64))[..., 0].view(np.uint32))


def test_valmetrics_spec_errors():
    from textualdegremoval_amd.metrics import ValMetrics
    with pytest.raises(ValueError, match='calculate_niqe'):
        ValMetrics({'niqe': {'type': 'calculate_niqe', 'crop_border': 0}})
    with pytest.raises(ValueError, match='use_image'):
        ValMetrics({'psnr': {'type': 'calculate_psnr', 'crop_border': 0}}, use_image=False)
    with pytest.raises(ValueError, match='input_order'):
        ValMetrics({'psnr': {'type': 'calculate_psnr', 'crop_border': 0, 'input_order': 'WHC'}})
    with pytest.raises(ValueError):
        ValMetrics({})


def test_valmetrics_means_equal_the_host_loop():
    """PSNR entries (plain, cropped, Y) through ValMetrics with the numpy reference as the kernel, against the validation loop's own
    arithmetic: `results[name] += fn(...)` per image, `/= cnt` at the end.  One image is identical to its ground truth (inf)."""
    from textualdegremoval_amd.metrics import ValMetrics, calculate_psnr
    spec = {'psnr': {'type': 'calculate_psnr', 'crop_border': 0, 'test_y_channel': False},
            'psnr_c4': {'type': 'calculate_psnr', 'crop_border': 4, 'test_y_channel': False, 'input_order': 'HWC'}}
    calls = []

    def stand_in(pred, gt, crop_border=0, swap_rb=True, what=(), want_y=False):
        calls.append((crop_border, tuple(what)))
        return torch.from_numpy(VR.rows(pred.numpy(), gt.numpy(), crop_border, swap_rb))

    rng = np.random.default_rng(11)
    for kinds in (('rgb',) * 5, ('rgb', 'same', 'rgb')):
        vm = ValMetrics(spec, kernel=stand_in)
        want = {m: 0 for m in spec}
        use = [_images(rng, k, 24, 40) for k in kinds]
        for a, b in use:
            vm.add(torch.from_numpy(a), torch.from_numpy(b), rgb2bgr=True)
            want['psnr'] += calculate_psnr(a[0], b[0], 0)
            want['psnr_c4'] += calculate_psnr(a[0], b[0], 4)
        got = vm.result()
        for m in want:
            want[m] /= len(use)
            assert _bits(got[m]) == _bits(want[m]), (m, got[m], want[m])
            assert len(vm.per_image[m]) == len(use)
        assert list(got) == list(spec)
    assert calls[:2] == [(0, ('psnr',)), (4, ('psnr',))]                                   # one call per crop, the union of its metrics


def test_float_sources_quantise_as_tensor2img():
    """the reference's quantisation of a float source (swap included) is tensor2img's, so the stand-in path above covers floats too"""
    from textualdegremoval_amd.metrics import tensor2img
    g = torch.Generator().manual_seed(3)
    x = torch.rand(1, 3, 9, 13, generator=g) * 1.2 - 0.1
    k = torch.arange(256, dtype=torch.float32)
    x[0, 0, 0, :8] = ((k[:8] + 0.5) / 255)                                                 # ties
    for swap in (False, True):
        assert np.array_equal(VR.quantise(x, swap)[0], tensor2img(x, rgb2bgr=swap))
