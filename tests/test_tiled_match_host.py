"""Matched tiled inference, the parts that need no GPU: the window grid of a ref (dino.window_grid), the two entry points in the binding,
and the `val: {tile, tile_match}` plumbing of the step model against a stub session."""
import ctypes

import pytest
import torch


def test_window_grid_values_and_errors():
    from textualdegremoval_amd.dino import window_grid
    assert window_grid(192, 256, 128) == (3, 5, 32)
    assert window_grid(128, 384, 128) == (1, 9, 32)
    assert window_grid(128, 128, 128) == (1, 1, 32)
    assert window_grid(720, 1280, 256) == (8, 17, 64)
    assert window_grid(96, 128, 48) == (5, 7, 12)
    for Hr, Wr in ((100, 256), (256, 100), (64, 64)):
        with pytest.raises(ValueError) as e:
            window_grid(Hr, Wr, 128)
        assert f'{Hr} x {Wr}' in str(e.value) and '128 x 128' in str(e.value)


def test_entry_points_are_bound_and_exported():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    S = _lib.SIGNATURES
    assert 'tdr_window_resize_bilinear' in S and 'tdr_token_match_bank' in S
    for name in ('tdr_window_resize_bilinear', 'tdr_token_match_bank'):
        assert hasattr(lib, name), f'{name} is not exported by the built library'
        res, args = S[name]
        assert res is ctypes.c_int
        ptr = [a is ctypes.c_void_p or issubclass(a, ctypes._Pointer) for a in args]
        assert any(ptr) and all(p or a is ctypes.c_int for a, p in zip(args, ptr)), name      # pointers and ints, no struct
    assert len(S['tdr_window_resize_bilinear'][1]) == 13 and len(S['tdr_token_match_bank'][1]) == 21
    assert _lib.ABI_VERSION == 112


class _Stub:
    def __init__(self):
        self.calls = []

    def run_tiled(self, *a, **kw):
        self.calls.append((a, kw))
        return a[0]


def _model(val, net_ext):
    from textualdegremoval_amd.models.image_restoration_ref_model import RefGuidedImageCleanModel
    m = object.__new__(RefGuidedImageCleanModel)
    m.opt = {'val': val}
    m.net_g = torch.nn.Identity()
    m.net_ext = net_ext
    m.lq, m.ref = torch.zeros(1, 3, 64, 64), torch.zeros(1, 3, 96, 96)
    stub = _Stub()
    m._val_session = lambda net: stub
    return m, stub


def test_val_tile_match_reaches_run_tiled():
    matcher = object()
    m, stub = _model(dict(tile=48, tile_overlap=16, tile_batch=2, tile_match=True), matcher)
    m.nonpad_test()
    (a, kw), = stub.calls
    assert a[0] is m.lq and a[1] is m.ref and kw == dict(tile=48, overlap=16, tile_batch=2, matcher=matcher)
    assert m.output is m.lq
    m, stub = _model(dict(tile=48), matcher)                                  # without the key: the call as it was
    m.nonpad_test()
    assert stub.calls[0][1] == dict(tile=48, overlap=32, tile_batch=4)


def test_val_tile_match_needs_the_matcher_and_a_tile():
    m, stub = _model(dict(tile=48, tile_match=True), None)
    with pytest.raises(ValueError, match='path.pretrain_dino'):
        m.nonpad_test()
    m, stub = _model(dict(tile_match=True), object())
    with pytest.raises(ValueError) as e:
        m.nonpad_test()
    assert 'tile_match' in str(e.value) and 'val.tile ' in str(e.value) and not stub.calls
