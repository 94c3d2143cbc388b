"""Host-side checks of the inference path of the Restormer family (no GPU): `keep` is threaded through every forward function of the
three engines, tdr_attn_fold_proj is declared, exported and checks its arguments before launching, and the modules refuse host tensors
on the no-grad route as they do on the autograd route."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_forward_functions_of_the_three_engines_take_keep():
    from textualdegremoval_amd import drsformer_engine as DE, promptir_engine as PE, restormer_engine as R
    fns = [R.tblock_fwd, R.fblock_fwd, R.seq_fwd, R.refine_fwd, R.walk_fwd, R.net_fwd, R.attn_tail_fwd,
           PE.prompt_fwd, PE._prompt_stage_fwd, PE.net_fwd,
           DE.attn_fwd, DE.ffn_fwd, DE.tblock_fwd, DE.mefc_fwd, DE.net_fwd]
    for f in fns:
        p = inspect.signature(f).parameters.get('keep')
        assert p is not None and p.default is True, f'{f.__module__}.{f.__name__}'
    # every public *_fwd of the three engines that returns (out, saved) is in the list: none was forgotten
    listed = {f for f in fns}
    for mod in (R, PE, DE):
        for name, f in vars(mod).items():
            if name.endswith('_fwd') and not name.startswith('_') and inspect.isfunction(f) and f.__module__ == mod.__name__ \
                    and name not in ('down_fwd', 'up_fwd'):                    # (Downsample / Upsample return a tensor, save nothing)
                assert f in listed, f'{mod.__name__}.{name}'
    assert R.INFER_FOLD is True                            # module switch (A/B in profiles/probe_restormer_infer.py), no environment knob
    # the stage wrappers of DRSformer's MEFC sub-networks hand `keep` on
    seen = {}
    stage = DE._stage(lambda x, P, pre, **kw: seen.update(kw, pre=pre) or (x, None), 'refinement.')
    assert stage(1, {}, {}, keep=False) == (1, None) and seen == {'keep': False, 'pre': 'refinement.'}


def test_header_declares_and_library_exports_the_fold():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, 'include', 'tdr.h')).read()
    assert 'tdr_attn_fold_proj' in _lib.SIGNATURES
    assert hasattr(lib, 'tdr_attn_fold_proj'), 'tdr_attn_fold_proj is not exported by the built library'
    assert re.search(r'^int tdr_attn_fold_proj\(const float\* AT, const float\* Wo, int N, int C, int heads, float\* Wf, void\* stream\);',
                     txt, re.M), 'tdr_attn_fold_proj is not declared in include/tdr.h'


def test_fold_checks_its_arguments_before_launching():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    assert lib.tdr_attn_fold_proj(None, 64, 1, 48, 1, 64, None) != 0 and 'null pointer' in lib.tdr_last_error().decode()
    assert lib.tdr_attn_fold_proj(64, 64, 1, 48, 5, 128, None) != 0 and 'C % heads' in lib.tdr_last_error().decode()
    assert lib.tdr_attn_fold_proj(64, 64, 1, 400, 2, 128, None) != 0 and 'C/heads <= 192' in lib.tdr_last_error().decode()
    assert lib.tdr_attn_fold_proj(64, 64, 1, 48, 1, 64, None) != 0 and 'alias' in lib.tdr_last_error().decode()


def test_no_grad_route_is_shared_and_has_no_cpu_fallback(monkeypatch):
    """one function serves every arch module; under torch.no_grad() the Restormer-family modules do not enter their autograd node, and
    the route they take instead checks the device as the node does: a missing GPU is an error, never eager PyTorch"""
    from textualdegremoval_amd.models.archs import (define_network, nafnet_arch_utils as U, network_drsformer_guided_200L_SPA_arch as D2,
                                                    network_drsformer_guided_arch as D, network_nafnet_guided_arch as N,
                                                    network_promptir_guided_arch as PA, network_restormer_guided_arch as RA)
    assert N._infer_fwd is U.infer_fwd and all(m.infer_fwd is U.infer_fwd for m in (RA, PA, D, D2))

    def entered(*a, **k):
        raise AssertionError('the autograd node was entered under torch.no_grad()')
    for m in (RA, PA, D, D2):
        monkeypatch.setattr(m._NetFn, 'apply', entered)
    monkeypatch.setattr(RA._UNetFn, 'apply', entered)
    x = torch.rand(1, 3, 16, 16)
    small = dict(dim=8, num_blocks=[1, 1, 1, 1], heads=[1, 1, 1, 1])
    guided = dict(small, nf=8, ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1])
    for opt, images in ((dict(type='Restormer', num_refinement_blocks=1, **small), (x,)),
                        (dict(type='RestormerRefFusion', num_refinement_blocks=1, **guided), (x, x)),
                        (dict(type='DRSformer', **small), (x,)),
                        (dict(type='DRSformerRefFusion', **guided), (x, x)),
                        (dict(type='DRSformer200L_SPA_RefFusion', **guided), (x, x)),
                        (dict(type='PromptIR', dim=48, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, decoder=True), (x,))):
        net = define_network(opt)
        with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):
            net(*images)
