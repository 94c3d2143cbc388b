"""Host-side checks of NAFNetDynamicFusion (no GPU): the module tree against the reference's (tests/golden/dynfusion.npz,
make_golden_dynfusion.py), the architecture registry after the new module joined it, and the two reference defects R10 / R11."""
import os

import numpy as np
import pytest
import torch

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'dynfusion.npz'))
CFG = dict(img_channel=3, width=8, middle_blk_num=1, enc_blk_nums=[1, 1, 2], dec_blk_nums=[1, 1, 1])


def test_parameter_names_shapes_and_order():
    from textualdegremoval_amd.models.archs import define_network
    net = define_network(dict(type='NAFNetDynamicFusion', **CFG))
    assert [k for k, _ in net.named_parameters()] == [str(n) for n in G['names']]
    assert [str(list(p.shape)) for _, p in net.named_parameters()] == [str(s) for s in G['shapes']]
    assert list(net.state_dict().keys()) == [str(n) for n in G['names']]
    sd = net.state_dict()
    assert sd['encoders.0.layers.0.kernel.0.weight'].shape == (16, 10240)
    assert sd['encoders.0.layers.0.sg1.kernel.0.weight'].shape == (32, 10240)
    assert 'encoders.0.layers.0.kernel.0.bias' not in sd and 'middle_blks.layers.0.sg2.kernel.0.bias' not in sd


def test_default_init_matches_reference_construction():
    """same module construction order as the reference: under one seed the projection weights are the Linear default init"""
    from textualdegremoval_amd.models.archs.network_nafnet_guided_diffir_arch import NAFNetDynamicFusion
    torch.manual_seed(0)
    a = NAFNetDynamicFusion(**CFG)
    torch.manual_seed(0)
    b = NAFNetDynamicFusion(**CFG)
    w = a.state_dict()['middle_blks.layers.0.kernel.0.weight']
    assert torch.equal(w, b.state_dict()['middle_blks.layers.0.kernel.0.weight'])
    assert w.abs().max().item() <= 1.0 / 10240 ** 0.5
    assert float(a.encoders[0].layers[0].beta.detach().abs().max()) == 0.0


def test_registry_resolves_every_existing_type_as_before():
    """define_network takes the first match in sorted module order; network_nafnet_guided_arch sorts before
    network_nafnet_guided_diffir_arch, so the names both define (NAFNet, NAFBlock, SimpleGate, NAFNetLocal) keep resolving there"""
    import torch.nn as nn
    from textualdegremoval_amd.models import archs
    mods = archs._arch_modules
    names = [m.__name__.rsplit('.', 1)[1] for m in mods]
    assert names.index('network_nafnet_guided_arch') < names.index('network_nafnet_guided_diffir_arch')
    old = [m for m in mods if not m.__name__.endswith('network_nafnet_guided_diffir_arch')]
    types = {k for m in old for k, v in vars(m).items() if isinstance(v, type) and issubclass(v, nn.Module)}
    assert {'NAFNet', 'NAFNetRefFusion', 'NAFNetLocal', 'Restormer', 'SFNet'} <= types
    for t in sorted(types):
        before = next(getattr(m, t) for m in old if getattr(m, t, None) is not None)
        after = next(getattr(m, t) for m in mods if getattr(m, t, None) is not None)
        assert after is before, t
    from textualdegremoval_amd.models.archs import network_nafnet_guided_arch as g
    assert archs.dynamic_instantiation(mods, 'NAFNet', dict(width=8, enc_blk_nums=[1], dec_blk_nums=[1])).__class__ is g.NAFNet
    from textualdegremoval_amd.models.archs import network_nafnet_guided_diffir_arch as d
    assert archs.dynamic_instantiation(mods, 'NAFNetDynamicFusion', dict(CFG)).__class__ is d.NAFNetDynamicFusion


def test_r11_nafnet_local_dynamic_raises_type_error():
    from textualdegremoval_amd.models.archs import define_network
    with pytest.raises(TypeError) as e:
        define_network(dict(type='NAFNetLocalDynamic', **CFG))
    assert str(G['r11_error']) in str(e.value)


def test_r10_twenty_word_embedding_raises():
    """DiffIRRefGuidedImageCleanModel builds Mapper(num_words=20): k_v [N, 20, 1024] against Linear(10 * 1024, .)"""
    from textualdegremoval_amd.models.archs import define_network
    assert 'mat1 and mat2 shapes cannot be multiplied (1x20480 and 10240x' in str(G['r10_error'])
    net = define_network(dict(type='NAFNetDynamicFusion', **CFG))
    with pytest.raises(RuntimeError) as e:
        net(torch.rand(1, 3, 32, 32), torch.randn(1, 20, 1024))
    assert 'mat1 and mat2 shapes cannot be multiplied (1x20480 and 10240x' in str(e.value)


def test_unsupported_block_options_raise():
    from textualdegremoval_amd.models.archs.network_nafnet_guided_diffir_arch import NAFBlock_DynamicFusion
    with pytest.raises(NotImplementedError):
        NAFBlock_DynamicFusion(8, drop_out_rate=0.1)
    with pytest.raises(NotImplementedError):
        NAFBlock_DynamicFusion(8, FFN_Expand=3)
