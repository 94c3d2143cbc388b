"""The float64 MASA reference that tests/test_hip_masa_kernels.py leans on (tests/_masa_ref.py), pinned on the CPU: in float64 it
reproduces the reference project's recorded float32 results (tests/golden/masa_ops.npz) to 4 float32 ulp of each tensor's maximum,
and every input builder obeys the preconditions of the kernels (index range, -size <= start, start + side <= size when the map is
at least a block wide) and the margin the planted arg-max rows promise."""
import os

import numpy as np
import pytest
import torch

import _masa_ref as MR
from oracle import nafnet_ref_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def gold():
    g = np.load(os.path.join(GOLDEN, 'masa_ops.npz'))
    return {k: torch.from_numpy(g[k]) for k in g.files}


def close(a, golden):
    return MR.maxabs(a, golden) <= MR.floor_bar(golden)


@pytest.mark.parametrize('s', [1, 2, 4])
def test_transfer_ref_reproduces_golden(gold, s):
    fea, att, idx, go = (gold[f'tr{s}_{k}'] for k in ('fea', 'att', 'idx', 'go'))
    B = fea.shape[0]
    z = torch.zeros(B, 1, dtype=torch.long)
    out, dfeat, datt = MR.transfer_ref(fea, z, z, idx.view(B, 64), att.view(B, 64), 1, 1, 8, 15, s, go, torch.float64)
    assert close(out, gold[f'tr{s}_out'])
    assert close(dfeat, gold[f'tr{s}_gfea'])
    assert close(datt.view(B, 1, 8, 8), gold[f'tr{s}_gatt'])


def test_fine_bwd_ref_reproduces_golden(gold):
    B = gold['so_lr'].shape[0]
    att, invq, invk, dlrb, drefb = MR.fine_bwd_ref(gold['so_lr'], gold['so_ref'], gold['so_idx'].view(B, 64), gold['so_go'].view(B, 64),
                                                   torch.float64)
    assert close(att.view(B, 8, 8), gold['so_val'])
    assert close(dlrb, gold['so_glr'])
    assert close(drefb, gold['so_gref'])
    assert invq.shape == (B, 64) and invk.shape == (B, 169)
    # the reciprocal norms are the ones of the similarity: att = <q, k> invq invk at the selected patch
    q = torch.nn.functional.unfold(gold['so_lr'].double(), 3).transpose(1, 2)
    k = torch.nn.functional.unfold(gold['so_ref'].double(), 3)
    sel = k.gather(2, gold['so_idx'].view(B, 1, 64).expand(B, k.shape[1], 64)).transpose(1, 2)
    again = (q * sel).sum(2) * invq * invk.gather(1, gold['so_idx'].view(B, 64))
    assert MR.maxabs(again, att) < 1e-14


def test_argmax_ref_reproduces_golden(gold):
    dots, invq, invk = MR.coarse_products(gold['cs_lr'], gold['cs_ref'], [1, 2, 3])
    idx, val = MR.argmax_ref(dots, invq, invk)
    assert torch.equal(idx, gold['cs_idx'])
    assert close(val, gold['cs_val'])
    # the fine layout against the recorded fine search (max and gather agree at the recorded index)
    B = gold['so_lr'].shape[0]
    q = torch.nn.functional.unfold(gold['so_lr'].double(), 3).transpose(1, 2)
    k = torch.nn.functional.unfold(gold['so_ref'].double(), 3)
    fidx, fval = MR.argmax_ref(torch.bmm(q, k), 1.0 / q.norm(dim=2), 1.0 / k.norm(dim=1))
    assert torch.equal(fidx.view(B, 8, 8), gold['so_idx'])
    assert close(fval.view(B, 8, 8), gold['so_val'])


def test_argmax_ref_takes_the_first_of_equal_maxima():
    dots = torch.tensor([[[1., 4., 4., 0.], [4., -1., 4., 4.]]])
    idx, val = MR.argmax_ref(dots, torch.ones(1, 2), torch.ones(1, 4))
    assert idx.tolist() == [[1, 0]] and val.tolist() == [[4., 4.]]


# ------------------------------------------------------------------------------------------------------------ builders
@pytest.mark.parametrize('kind', MR.INDEX_PATTERNS)
@pytest.mark.parametrize('K,R1', [(8, 13), (12, 19), (8, 7)])
def test_index_patterns(kind, K, R1):
    if kind == 'coherent' and K > R1:
        with pytest.raises(AssertionError):
            MR.index_pattern(kind, 3, K, R1, 0)
        return
    idx = MR.index_pattern(kind, 5, K, R1, 3)
    assert idx.shape == (5, K * K) and idx.dtype == torch.long and idx.is_contiguous()
    assert int(idx.min()) >= 0 and int(idx.max()) < R1 * R1
    assert torch.equal(idx, MR.index_pattern(kind, 5, K, R1, 3))                  # seeded
    if kind == 'coherent':
        v = idx.view(5, K, K)
        assert ((v[:, 1:] - v[:, :-1]) == R1).all() and ((v[:, :, 1:] - v[:, :, :-1]) == 1).all()
    if kind == 'constant':
        assert (idx == idx[:, :1]).all()
    if kind == 'corners':
        assert set(idx.unique().tolist()) <= {0, R1 - 1, R1 * (R1 - 1), R1 * R1 - 1} and idx.unique().numel() == 4


@pytest.mark.parametrize('geom', sorted(MR.TRANSFER_GEOM))
def test_boxes_obey_the_gather_preconditions(geom):
    N, C, py, px, K, side, Hd, Wd = MR.TRANSFER_GEOM[geom]
    y1, x1 = MR.boxes(N, py * px, Hd, Wd, side)
    assert y1.shape == x1.shape == (N, py * px)
    for start, size in ((y1, Hd), (x1, Wd)):
        assert (start >= -size).all()                          # one python wrap at the most
        assert (start + side <= size).all()                    # never past the far edge
        if size >= side:
            assert (start >= 0).all()
    if py * px >= 2:
        assert torch.equal(y1[:, 0], y1[:, -1]) and torch.equal(x1[:, 0], x1[:, -1])      # two blocks of an image share a box
    if geom == 'A':
        assert (y1 < 0).all() and (x1 >= 0).all() and x1.unique().numel() == 3           # negative starts on one axis only
        O.gather_ref_block(torch.zeros(N, 1, Hd, Wd), y1, x1, side, 1)                   # the reference accepts them


@pytest.mark.parametrize('geom,s,pattern', MR.TRANSFER_CASES)
def test_transfer_inputs(geom, s, pattern):
    i = MR.transfer_inputs(geom, s, pattern)
    N, C, py, px, K, side, Hd, Wd = MR.TRANSFER_GEOM[geom]
    B = N * py * px
    assert i['feat'].shape == i['dfeat_pre'].shape == (N, C, Hd * s, Wd * s)
    assert i['dout'].shape == (N, C, py * K * s, px * K * s)
    assert i['index_all'].shape == i['soft_att'].shape == i['datt_pre'].shape == (B, K * K)
    assert 0 <= int(i['index_all'].min()) and int(i['index_all'].max()) < (side - 2) ** 2
    assert 0.2 <= float(i['soft_att'].min()) and float(i['soft_att'].max()) <= 1.0
    # every source pixel a patch can name lies inside the wrapped block: rows [y1 s, (y1 + side) s) with one wrap at the most
    assert (i['y1'] * s >= -Hd * s).all() and ((i['y1'] + side) * s <= Hd * s).all()
    assert (i['x1'] * s >= -Wd * s).all() and ((i['x1'] + side) * s <= Wd * s).all()


def test_transfer_case_list_is_what_the_kernels_need():
    cases = set(MR.TRANSFER_CASES)
    assert len(cases) == len(MR.TRANSFER_CASES)
    want = {'A': (1, 2, 4, 8, 16), 'B': (1, 2), 'C': (1, 4), 'D': (1, 2)}
    for geom, scales in want.items():
        for s in scales:
            pats = {p for g, ss, p in cases if g == geom and ss == s}
            assert 'random' in pats and len(pats) >= 2
    assert {p for g, s, p in cases if g == 'A' and s == 2} == set(MR.INDEX_PATTERNS)
    assert {(g, s) for g, s, p in cases} == {(g, s) for g, sc in want.items() for s in sc}


@pytest.mark.parametrize('B,P,R', [(1, 5, 49), (7, 1, 169), (3, 3, 361)])
def test_fine_argmax_builders(B, P, R):
    dots, invq, invk, cols = MR.fine_argmax_inputs(B, P, R)
    v = MR.argmax_products(dots, invq, invk)
    idx, val = MR.argmax_ref(dots, invq, invk)
    assert torch.equal(idx, cols)
    others = v.abs().scatter(2, cols.unsqueeze(2), 0.0).max(dim=2).values
    assert (val >= MR.PLANT_MARGIN * others).all()                               # the stated margin
    assert {0, R - 1} <= set(cols.view(-1).tolist()) and (R <= 64 or int(cols.max()) >= 64)
    dots, invq, invk, first = MR.fine_argmax_tie_inputs(B, P, R)
    v = MR.argmax_products(dots, invq, invk)
    assert ((v == 5).sum(dim=2) >= 2).all() and float(v.max()) == 5.0           # an exact, repeated maximum in every row
    assert torch.equal(MR.argmax_ref(dots, invq, invk)[0], first)


@pytest.mark.parametrize('Hr,Wr', MR.COARSE_MAPS)
def test_coarse_argmax_builders(Hr, Wr):
    dots, invq, invk, cols = MR.coarse_argmax_inputs(Hr, Wr)
    v = MR.argmax_products(dots, invq, invk)
    idx, val = MR.argmax_ref(dots, invq, invk)
    assert torch.equal(idx, cols)
    others = v.abs().scatter(2, cols.unsqueeze(2), 0.0).max(dim=2).values
    assert (val >= MR.PLANT_MARGIN * others).all()
    ys, xs = cols.view(-1) // Wr, cols.view(-1) % Wr
    corners = {(0, 0), (0, Wr - 1), (Hr - 1, 0), (Hr - 1, Wr - 1)}
    got = set(zip(ys.tolist(), xs.tolist()))
    assert corners <= got
    assert any(y == 0 and 0 < x < Wr - 1 for y, x in got) and any(y == Hr - 1 and 0 < x < Wr - 1 for y, x in got)
    assert any(x == 0 and 0 < y < Hr - 1 for y, x in got) and any(x == Wr - 1 and 0 < y < Hr - 1 for y, x in got)
    assert any(0 < y < Hr - 1 and 0 < x < Wr - 1 for y, x in got)
    for dia in (7, 13):                                                          # all four clamps of box_start are reached
        for c, size in ((ys, Hr), (xs, Wr)):
            b = O.box_start(c, size, dia)
            assert (b >= -size).all() and (b + dia + 2 <= size).all()
    dots, invq, invk, first = MR.coarse_argmax_tie_inputs(Hr, Wr)
    v = MR.argmax_products(dots, invq, invk)
    assert ((v == 15).sum(dim=2) >= 2).all() and float(v.max()) == 15.0
    assert torch.equal(MR.argmax_ref(dots, invq, invk)[0], first)


@pytest.mark.parametrize('B,C,K,D', MR.FINE_BWD_CASES)
def test_fine_bwd_inputs(B, C, K, D):
    for pattern in MR.FINE_BWD_PATTERNS:
        i = MR.fine_bwd_inputs(B, C, K, D, pattern)
        assert i['lrb'].shape == (B, C, K + 2, K + 2) and i['refb'].shape == (B, C, D, D)
        assert 0 <= int(i['index_all'].min()) and int(i['index_all'].max()) < (D - 2) ** 2
