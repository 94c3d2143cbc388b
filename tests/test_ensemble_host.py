"""The definition of the geometric self-ensemble (inference.dihedral / dihedral_inverse / ensemble_ops) on CPU tensors, and the two
entry points of csrc/tdr_dihedral.hip in the header.  No GPU."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ensemble_ops_values_and_errors():
    from textualdegremoval_amd.inference import ensemble_ops
    assert ensemble_ops(8) == (0, 1, 2, 3, 4, 5, 6, 7)
    assert ensemble_ops(4) == (0, 1, 2, 3)
    assert ensemble_ops(2) == (0, 1)
    assert ensemble_ops(1) == (0,)
    assert ensemble_ops([5, 0, 5, 3]) == (0, 3, 5)
    assert ensemble_ops((7,)) == (7,)
    assert ensemble_ops(iter([6, 1])) == (1, 6)
    for bad in (0, 3, 5, 16, -1, (), [], [8], [-1], [0, 9], None, 2.0, [1.0], 'x'):
        with pytest.raises(ValueError):
            ensemble_ops(bad)


def test_dihedral_follows_the_bit_definition():
    from textualdegremoval_amd.inference import dihedral
    x = torch.arange(2 * 3 * 5 * 7, dtype=torch.float32).view(2, 3, 5, 7)
    assert dihedral(x, 0) is x
    assert torch.equal(dihedral(x, 1), x.flip(-1)) and torch.equal(dihedral(x, 2), x.flip(-2))
    assert torch.equal(dihedral(x, 3), x.flip(-1).flip(-2))
    for op in range(4):
        assert torch.equal(dihedral(x, 4 + op), dihedral(x, op).transpose(-2, -1))          # the transpose comes after the flips
    assert dihedral(x, 5)[1, 2, 0, 0] == x[1, 2, 0, 6] and dihedral(x, 6)[1, 2, 0, 0] == x[1, 2, 4, 0]


def test_inverse_undoes_every_op():
    from textualdegremoval_amd.inference import dihedral, dihedral_inverse
    x = torch.randn(2, 3, 5, 7, generator=torch.Generator().manual_seed(1))
    for op in range(8):
        y = dihedral(x, op)
        assert tuple(y.shape) == ((2, 3, 7, 5) if op >= 4 else (2, 3, 5, 7))
        assert torch.equal(dihedral_inverse(y, op), x)
        assert torch.equal(dihedral_inverse(y.contiguous(), op), x)


def test_the_eight_transforms_of_an_asymmetric_image_differ():
    from textualdegremoval_amd.inference import dihedral
    x = torch.randn(1, 1, 6, 6, generator=torch.Generator().manual_seed(2))               # (square: all eight have one shape)
    outs = [dihedral(x, op).contiguous() for op in range(8)]
    for a in range(8):
        for b in range(a + 1, 8):
            assert not torch.equal(outs[a], outs[b]), (a, b)


def test_header_declares_the_dihedral_entry_points():
    txt = open(os.path.join(ROOT, 'include', 'tdr.h')).read()
    head = txt[:txt.index('#define TDR_ABI_VERSION')]
    assert 'tdr_dihedral_gather / tdr_dihedral_mean' in head                               # (listed among the additions to ABI 112)
    assert re.search(r'#define TDR_ABI_VERSION 112\b', txt)
    code = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    syms = set(re.findall(r'\b(tdr_[a-z0-9_]+)\s*\(', code))
    assert {'tdr_dihedral_gather', 'tdr_dihedral_mean'} <= syms
    from textualdegremoval_amd import _lib
    lib = _lib.load()                                                                      # raises if a declared symbol is missing
    for s in ('tdr_dihedral_gather', 'tdr_dihedral_mean'):
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['tdr_dihedral_gather'][1]) == 10 and len(_lib.SIGNATURES['tdr_dihedral_mean'][1]) == 12
    assert lib.tdr_dihedral_gather(None, 0, 1, 1, 4, 4, 0, 0x11, None, None) != 0          # a mixed mask: an error code, no launch
    assert 'mixes' in lib.tdr_last_error().decode()
    assert lib.tdr_dihedral_mean(None, 0, None, 0, 1, 1, 4, 4, None, None, 0, None) != 0   # no op selected
