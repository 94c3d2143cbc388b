"""Host-side checks of the inference path of NAFNetDynamicFusion (no GPU): the three forward-only launches of the modulated block are
exported and declared, their arguments are checked before anything is launched, the engine's forward functions take `keep`, and the
modules take the no-grad path without entering their autograd node -- and refuse host tensors there as the node does."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = (('tdr_dyn_head_infer', 'TdrDynHeadDesc'), ('tdr_dyn_dwsg_fwd', 'TdrDynDwsgDesc'), ('tdr_dyn_tail_infer', 'TdrDynTailDesc'))


def test_library_exports_and_header_declares_the_three_launches():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, 'include', 'tdr.h')).read()
    for s, desc in SYMBOLS:
        assert s in _lib.SIGNATURES
        assert _lib.SIGNATURES[s][1][0]._type_ is getattr(_lib, desc)
        assert hasattr(lib, s), f'{s} is not exported by the built library'
        assert re.search(r'^int ' + s + r'\(const ' + desc + r'\* d, void\* stream\);', txt, re.M), f'{s} is not declared in include/tdr.h'
        assert re.search(r'^} ' + desc + ';', txt, re.M)


def _filled(desc):
    """every pointer field set to a 16-byte aligned dummy (never dereferenced: the argument checks return first)"""
    d = desc()
    for name, typ in desc._fields_:
        if typ is C.c_void_p:
            setattr(d, name, 64)
    return d


def _shape(d, c, n=1):
    d.N, d.C = n, c
    if hasattr(d, 'HW'):
        d.HW, d.w_fmt = 64, 1
    else:
        d.H, d.W = 8, 8


def test_arguments_are_checked_on_the_host():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    for s, desc in SYMBOLS:
        fn, desc = getattr(lib, s), getattr(_lib, desc)
        d = desc()                                                   # all NULL
        assert fn(C.byref(d), None) != 0 and 'null pointer' in lib.tdr_last_error().decode(), s
        d = _filled(desc)
        _shape(d, 48)                                                # the support predicate is tdr_naf_tail_supported's
        assert fn(C.byref(d), None) != 0 and 'needs C in {32, 64, 128, 256}' in lib.tdr_last_error().decode(), s
        d = _filled(desc)
        _shape(d, 32, n=17)
        assert fn(C.byref(d), None) != 0 and 'N <= 16' in lib.tdr_last_error().decode(), s


def test_engine_forward_functions_take_keep():
    from textualdegremoval_amd import dynfusion_engine as D
    for f in (D.dyn_naf_fwd, D.dyn_unet_fwd, D._seq_fwd):
        p = inspect.signature(f).parameters.get('keep')
        assert p is not None and p.default is True, f.__name__
    assert D.INFER_KERNELS is True                                   # module switch (A/B in profiles/probe_dynfusion_infer.py), no environment knob


def test_no_grad_forward_bypasses_autograd_and_has_no_cpu_fallback(monkeypatch):
    from textualdegremoval_amd.models.archs import define_network, network_nafnet_guided_diffir_arch as A

    def entered(*a, **k):
        raise AssertionError('the autograd node was entered under torch.no_grad()')
    monkeypatch.setattr(A._DynNetFn, 'apply', entered)
    monkeypatch.setattr(A._DynBlockFn, 'apply', entered)
    net = define_network(dict(type='NAFNetDynamicFusion', width=8, enc_blk_nums=[1], dec_blk_nums=[1]))
    kv = torch.randn(1, 10, 1024)
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.rand(1, 3, 16, 16), kv)
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
        A.NAFBlock_DynamicFusion(16)(torch.rand(1, 16, 8, 8), kv)
    # nothing requires grad: the same path with grad mode on
    for p in net.parameters():
        p.requires_grad_(False)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.rand(1, 3, 16, 16), kv)
    # R10 stays in front: a 20-word embedding fails on its shape, not on the device
    with torch.no_grad(), pytest.raises(RuntimeError, match='cannot be multiplied'):
        net(torch.rand(1, 3, 16, 16), torch.randn(1, 20, 1024))
