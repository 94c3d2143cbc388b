"""Host-side checks of the inference path of the NAFNet family (no GPU): the forward-only NAFBlock chains are exported and declared,
their argument contract (the tensors they do not write must be NULL) is enforced before anything is launched, the engine's forward
functions take `keep`, and the modules refuse host tensors on the no-grad path as they do on the autograd path."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFER_SYMBOLS = ('tdr_naf_tail_infer', 'tdr_naf_head_infer')


def test_library_exports_and_header_declares_the_forward_only_chains():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, 'include', 'tdr.h')).read()
    for s in INFER_SYMBOLS:
        assert s in _lib.SIGNATURES
        assert hasattr(lib, s), f'{s} is not exported by the built library'
        assert re.search(r'^int ' + s + r'\(const \w+\* d, void\* stream\);', txt, re.M), f'{s} is not declared in include/tdr.h'
    # same descriptors as the training chains: nothing about the existing structs changes
    assert _lib.SIGNATURES['tdr_naf_tail_infer'] == _lib.SIGNATURES['tdr_naf_tail_fwd']
    assert _lib.SIGNATURES['tdr_naf_head_infer'] == _lib.SIGNATURES['tdr_naf_head_fwd']


def _filled(desc, skip):
    """every pointer field of a descriptor set to a dummy (never dereferenced: the argument checks return first) except `skip`"""
    d = desc()
    for name, typ in desc._fields_:
        if typ is C.c_void_p and name not in skip:
            setattr(d, name, 64)
    return d


def test_forward_only_chains_reject_the_saved_tensor_fields():
    """the tensors the chains do not write are NULL in their descriptors; a caller that hands one over (expecting it filled) is told so.
    The checks run on the host before any launch."""
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    for fn, desc, saved in ((lib.tdr_naf_tail_infer, _lib.TdrNafTailDesc, ('y', 'mu', 'rs', 'yn', 't4')),
                            (lib.tdr_naf_head_infer, _lib.TdrNafHeadFwdDesc, ('mu', 'rs', 'xn'))):
        d = desc()                                                   # all NULL
        assert fn(C.byref(d), None) != 0 and 'null pointer' in lib.tdr_last_error().decode()
        for s in saved:
            d = _filled(desc, [t for t in saved if t != s])
            d.N, d.C, d.HW, d.w_fmt = 1, 32, 64, 1
            assert fn(C.byref(d), None) != 0
            assert 'must be NULL' in lib.tdr_last_error().decode(), s
        d = _filled(desc, saved)
        d.N, d.C, d.HW, d.w_fmt = 1, 48, 64, 1                       # the support predicate is the training chains'
        assert fn(C.byref(d), None) != 0 and 'needs C in {32, 64, 128, 256}' in lib.tdr_last_error().decode()


def test_engine_forward_functions_take_keep():
    from textualdegremoval_amd import engine as E
    for f in (E.naf_fwd, E.naf_seq_fwd, E.encoder_fwd, E.pyramids_fwd, E.masa_fwd, E.walk_fwd, E.net_fwd, E.unet_fwd):
        p = inspect.signature(f).parameters.get('keep')
        assert p is not None and p.default is True, f.__name__
    assert E.INFER_KERNELS is True                                   # module switch (A/B in profiles/probe_infer.py), no environment knob


def test_kernel_wrappers_exist():
    from textualdegremoval_amd import kernels as K
    assert list(inspect.signature(K.naf_tail_infer).parameters) == list(inspect.signature(K.naf_tail_fwd).parameters)
    assert list(inspect.signature(K.naf_head_infer).parameters) == list(inspect.signature(K.naf_head_fwd).parameters)


def test_no_grad_forward_bypasses_autograd_and_has_no_cpu_fallback(monkeypatch):
    """under torch.no_grad() the modules do not enter their autograd node, and the path they take instead checks the device as the node
    does: a missing GPU is an error, never eager PyTorch"""
    from textualdegremoval_amd.models.archs import define_network, network_nafnet_guided_arch as A

    def entered(*a, **k):
        raise AssertionError('the autograd node was entered under torch.no_grad()')
    monkeypatch.setattr(A._UNetFn, 'apply', entered)
    monkeypatch.setattr(A._NetFn, 'apply', entered)
    x = torch.rand(1, 3, 16, 16)
    for net, images in ((define_network(dict(type='NAFNet', width=8, enc_blk_nums=[1], dec_blk_nums=[1])), (x,)),
                        (define_network(dict(type='NAFNetRefFusion', width=8, nf=8, enc_blk_nums=[1, 1, 1, 1], dec_blk_nums=[1, 1, 1, 1],
                                             ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1, 1])), (x, x))):
        with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
            net(*images)
