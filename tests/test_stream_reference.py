"""The float64 references and bars that tests/test_hip_stream_float64.py leans on (tests/_stream_ref.py), pinned on the CPU:
  1. in float64 the LayerNorm reference reproduces oracle.nafnet_ref_oracle.layernorm2d and its autograd to 1e-12;
  2. every bar can fail: one structural defect planted in the float64 reference (a pixel left out of gw / gb, a channel left out of the
     statistics, add applied to one channel too many, the uncentred yu in gw, one partial row dropped) moves the result past the bar
     of that very case -- a condition on the O(1) inputs, met by the defect-free reference alone;
  3. the input builders keep what they promise (the offset regime's 20 sigma, exact integer sums, exact dead pixels, exact Gram inputs
     of the SCA chain) and the dispatch tables reach the branches they name."""
import numpy as np
import pytest
import torch

import _stream_ref as SR
from _masa_ref import maxabs
from oracle import nafnet_ref_oracle as O


def ident(case):
    return '-'.join(str(v) for v in case)


# ------------------------------------------------------------------------------------------------------------------ reference
def test_ln_ref_reproduces_oracle_autograd():
    C, N, HW = 24, 2, 21
    inp = SR.ln_inputs(C, N, HW, 1, 'randn')
    x, w, b = (inp[k].double().clone().requires_grad_(True) for k in ('x', 'w', 'b'))
    y = O.layernorm2d(x, w, b, SR.EPS)
    y.backward(inp['go'].double())
    r = SR.ln_ref(inp['x'], inp['w'], inp['b'], inp['go'], None, 0, 1, torch.float64)
    for got, want in ((r['y'], y), (r['gx'], x.grad), (r['gw'], w.grad), (r['gb'], b.grad),
                      (r['mu'], x.detach().mean(1).view(N, HW)), (r['rstd'], 1 / torch.sqrt(x.detach().var(1, unbiased=False) + SR.EPS).view(N, HW))):
        assert maxabs(got, want) < 1e-12


def test_ln_ref_biasfree_and_add_against_autograd():
    """center = 0 (y = x rstd w with the variance about the mean) and the add on the first add_C channels"""
    C, N, HW = 24, 2, 21
    inp = SR.ln_inputs(C, N, HW, 0, 'offset', 'part', 0, 1)
    x, w = (inp[k].double().clone().requires_grad_(True) for k in ('x', 'w'))
    y = x / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + SR.EPS) * w.view(1, -1, 1, 1)
    y.backward(inp['go'].double())
    r = SR.ln_ref(inp['x'], inp['w'], None, inp['go'], SR.ln_add(inp), inp['add_C'], 0, torch.float64)
    want = x.grad.clone()
    want[:, :inp['add_C']] += SR.ln_add(inp)[:, :inp['add_C']].double()
    scale = y.detach().abs().max().item()
    assert maxabs(r['y'], y) < 1e-12 * scale and maxabs(r['gx'], want) < 1e-12 * scale
    assert maxabs(r['gw'], w.grad) < 1e-12 * w.grad.abs().max().item()
    assert maxabs(r['mu'], x.detach().mean(1).view(N, HW)) < 1e-12 * scale


# ------------------------------------------------------------------------------------------------------------- dispatch tables
def test_ln_tables_reach_every_branch():
    fwd = {SR.ln_fwd_kernel_name(C, N, HW) for C, N, HW, *_ in SR.LN_FWD_CASES}
    assert fwd == {'ln_fwd_kernel<4,8>', 'ln_fwd_kernel<4,16>', 'ln_fwd_kernel<4,32>', 'ln_fwd_kernel<8,32>', 'ln_fwd_kernel<16,32>',
                   'ln_fwd_narrow_kernel<12>', 'ln_fwd_narrow_kernel<24>', 'ln_fwd_generic_kernel'}
    # both generic conditions, both sides of the 512-tile boundary at C = 513
    assert any(C > 1536 for C, *_ in SR.LN_FWD_CASES)
    assert {SR.ln_tiles(N, HW) for C, N, HW, *_ in SR.LN_FWD_CASES if C == 513} >= {511, 512}
    assert SR.ln_fwd_kernel_name(513, 2, 16321) == 'ln_fwd_generic_kernel' and SR.ln_fwd_kernel_name(513, 1, 64 * 511 - 5) == 'ln_fwd_narrow_kernel<12>'
    assert {HW for _, _, HW, *_ in SR.LN_FWD_CASES} >= {1, 63, 64, 65, 90, 77, 257, 70}
    sliced = {SR.ln_fwd_kernel_name(C, N, HW) for C, N, HW, _, _, xs in SR.LN_FWD_CASES if xs and N > 1}
    assert sliced == fwd                                                          # every forward template: x sliced with N > 1
    by = {}
    for case in SR.LN_BWD_CASES:
        by.setdefault(SR.ln_bwd_kernel_name(*case[:3]), []).append(case)
    assert set(by) == {'ln_bwd_kernel<4,8>', 'ln_bwd_kernel<4,16>', 'ln_bwd_kernel<8,16>', 'ln_bwd_cached_kernel<16>', 'ln_bwd_cached_kernel<32>',
                       'ln_bwd_generic_kernel<true>', 'ln_bwd_generic_kernel<false>+ln_param_grad_kernel'}
    for name, cases in by.items():
        assert {c[3] for c in cases} == {0, 1}, name                              # both center values
        assert {c[5] for c in cases} == {'none', 'full', 'part'}, name            # add absent, full, add_C < C
        assert any(c[6] and c[1] > 1 for c in cases), name                        # x a channel slice whose image stride is used (N > 1)
        assert 'offset' in {c[4] for c in cases}, name
        if name.startswith('ln_bwd_kernel'):                                      # one trip and two trips of the persistent grid
            tiles = [SR.ln_tiles(c[1], c[2]) for c in cases]
            assert min(tiles) < 256 and any(256 < t < 512 for t in tiles), name
    assert any(c[7] and c[1] > 1 for c in SR.LN_BWD_CASES) and any(c[1] == 1 for c in SR.LN_BWD_CASES)
    assert {c[2] for c in SR.LN_BWD_CASES} >= {1, 63, 65}
    assert SR.ln_tiles(3, 148 * 148) == 1029 and (148 * 148) % 64 != 0
    assert {SR.ln_bwd_kernel_name(*c[:3]) for c in SR.LN_BWD_EXACT_GB} == set(by)


def test_other_tables_reach_every_branch():
    assert all(n <= 1024 for n, _ in SR.PAIR_SUM_ONE_STAGE) and all(n > 1024 for n, _ in SR.PAIR_SUM_TWO_STAGE)
    c2 = [2 * C for _, C in SR.PAIR_SUM_TWO_STAGE]
    assert any(v < 128 and v & (v - 1) for v in c2) and any(v < 256 and not v & (v - 1) for v in c2) and any(v >= 256 for v in c2)
    assert any(128 < v < 256 for v in c2)                                         # one slice below 256 columns
    assert [N * HW for N, HW, _ in SR.CHANSUM_CASES] == [90, 8191, 8193, 40000]
    paths = {name: SR.rows_path(*rest) for name, *rest in SR.ROWS_CASES}
    assert paths == {'float4': 'rows_kernel', 'odd_length': 'rows_scalar_kernel', 'odd_stride': 'rows_scalar_kernel',
                     'offset_pointer': 'rows_scalar_kernel', 'scalar_grid_stride': 'rows_scalar_kernel', 'float4_grid_stride': 'rows_kernel'}
    length = {name: rest[1] for name, *rest in SR.ROWS_CASES}
    assert length['scalar_grid_stride'] > SR.GRID and length['float4_grid_stride'] // 4 > SR.GRID
    assert all(SR.dw_geom(H, W)[1] >= 2 for _, _, H, W in SR.DW_CASES)
    assert SR.dw_geom(9, 1028) == (8, 2, 4) and SR.dw_geom(40, 2052) == (8, 3, 15)
    # second 256-column trip, colb = 2, the co >= C tail, ragged 64-wide tiles, Cout != Cin
    assert any(C > 256 for C in SR.SCA_C) and any(C % 4 for C in SR.SCA_C) and any(C % 64 for C in SR.SCA_C)
    assert any(co != ci for co, ci, _ in SR.PARAM_CASES) and any(ci > 256 for _, ci, _ in SR.PARAM_CASES) and any(e for *_, e in SR.PARAM_CASES)


# ------------------------------------------------------------------------------------------------------------ input builders
@pytest.mark.parametrize('case', [c for c in SR.LN_FWD_CASES + SR.LN_BWD_CASES if c[4] == 'offset'], ids=ident)
def test_offset_regime_is_twenty_sigma(case):
    """on the very tensor the kernel of that case sees"""
    C = case[0]
    inp = SR.ln_inputs(*case) if len(case) == 8 else SR.ln_inputs(*case[:5], 'none', case[5], backward=False)
    x = inp['x'].double()
    ratio = x.mean(1).abs() / x.std(1, unbiased=False)
    assert ratio.min().item() >= 20
    if C >= 64:                                          # the outlier channels: every seventh one 8 times as wide
        xc = x - x[:, 1::7].mean(1, keepdim=True)        # (without the pixel's offset)
        assert xc[:, ::7].std((0, 2, 3)).min() > 4 * xc[:, 1::7].std((0, 2, 3)).max()


def test_dead_pixels_are_exact():
    for C, N, HW, center, regime, *_ in SR.LN_FWD_CASES + SR.LN_BWD_CASES:
        if regime != 'dead':
            continue
        x = SR.ln_x(C, N, HW, regime, SR._gen(2))
        pix = SR.dead_pixels(N, HW)
        assert len({(n, p) for n, p, _ in pix}) == 2 and (N - 1, HW - 1) not in {(n, p) for n, p, _ in pix}
        for n, p, v in pix:
            assert (x[n, :, 0, p] == v).all()
    # every partial sum of C copies is a multiple of 0.5 below 2^24, and (C v) / C is v, in float32, for every C of the tables
    for C in sorted({c[0] for c in SR.LN_FWD_CASES + SR.LN_BWD_CASES}):
        for v in SR.DEAD_VALUES:
            run = np.cumsum(np.full(C, v, np.float32), dtype=np.float32)
            assert run.dtype == np.float32 and (run == v * np.arange(1, C + 1)).all() and run[-1] / np.float32(C) == np.float32(v)
    assert all(v * 2 == int(v * 2) for v in SR.DEAD_VALUES)


def test_integer_regime_sums_exactly():
    for nparts, C in SR.PAIR_SUM_CASES:
        part = SR.pair_sum_inputs(nparts, C, 'integer')
        assert part.abs().max() <= 8 and torch.equal(part, part.round())
        assert torch.equal(part.sum(0).double(), part.double().sum(0)) and part.abs().sum(0).max() < 2 ** 24
    for N, HW, _ in SR.CHANSUM_CASES:
        x = SR.channel_sum_inputs(N, HW, 'integer')
        assert torch.equal(x.sum((0, 2, 3)).double(), x.double().sum((0, 2, 3))) and x.abs().sum((0, 2, 3)).max() < 2 ** 24
    for name, *rest in SR.ROWS_CASES[:4]:
        src, dst = SR.rows_inputs(name, *rest)
        out = SR.rows_ref(src, dst, *rest, add=True)
        assert torch.equal(out.float().double(), out) and out.abs().max() <= 100


@pytest.mark.parametrize('C,N,regime', SR.SCA_CASES, ids=lambda v: str(v))
def test_sca_gram_inputs_are_exact_in_float32(C, N, regime):
    """the kernels take G3 = sum_p dy g, S3 and pooled in float32; the dyadic maps make them exact, so the references (which start from
    the maps) and the kernels see the same numbers"""
    inp = SR.sca_inputs(C, N, regime)
    for k in ('G3', 'S3', 'pooled'):
        assert torch.equal(inp[k].float().double(), inp[k])
    # the float32 einsum of any order gives the same G3
    assert torch.equal(torch.einsum('nohw,nihw->noi', inp['dy'], inp['g']).double(), inp['G3'])
    if regime == 'integer':          # ds = sum_co beta W3 G3 and dbsca = sum_n ds stay below 2^24 in magnitude: exact in any order
        terms = (inp['beta'].view(1, C, 1) * inp['w3'].view(1, C, C) * inp['G3']).abs().sum((0, 1))
        assert terms.max() < 2 ** 24 and torch.equal(inp['w3'], inp['w3'].round()) and torch.equal(inp['beta'], inp['beta'].round())


def test_param_gram_inputs_are_exact_in_float32():
    for case in SR.PARAM_CASES:
        inp = SR.param_inputs(*case)
        assert torch.equal(inp['G'].float().double(), inp['G']) and torch.equal(inp['S'].float().double(), inp['S'])
        assert inp['G'].shape == (case[0], case[1]) and inp['w'].shape[0] == case[0] + case[2]


# ------------------------------------------------------------------------------------------------------- every bar can fail
def _ln_defect_moves_past_bar(case):
    C, N, HW, center, regime, add, xs, as_ = case
    inp = SR.ln_inputs(*case)
    ref = SR.ln_reference(inp)
    seen = []

    def past(defect, keys, dead=False):
        bad = SR.ln_reference(inp, defect)
        m = 1 - ref['live'] if dead else ref['live']
        for k in keys:
            if k in ('gw', 'gb'):
                err, b = maxabs(bad[k], ref[k]), ref['bar'][k]
            else:
                err, b = maxabs(SR.masked(bad[k], m), SR.masked(ref[k], m)), (ref['bar_dead'] if dead else ref['bar'])[k]
            assert err > b, (defect, k, err, b)
            seen.append((defect, k))

    past('drop_pixel', ('gw', 'gb'))
    if C > 1:
        past('short_stats', ('y', 'mu', 'rstd', 'gx'))
        if inp['dead']:
            past('short_stats', ('mu',), dead=True)          # the 0.5 pixel: its mean moves by 0.5 / C
    if add == 'part':
        past('add_wide', ('gx',))
    if center:
        past('uncentred_gw', ('gw',))
    return seen


@pytest.mark.parametrize('case', SR.LN_BWD_CASES, ids=ident)
def test_ln_bars_can_fail(case):
    seen = _ln_defect_moves_past_bar(case)
    assert ('drop_pixel', 'gw') in seen and ('drop_pixel', 'gb') in seen


@pytest.mark.parametrize('case', SR.LN_FWD_CASES, ids=ident)
def test_ln_forward_bars_can_fail(case):
    """the forward-only table: the last channel left out of the statistics moves y, mu and rstd past their bars"""
    C, N, HW, center, regime, xs = case
    if N * C * HW > 4e6:
        # the two boundary cases are the 513-channel statistics of (513, 2, 77) at another pixel count: the per-pixel condition is the same
        C, N, HW = C, 1, 77
    inp = SR.ln_inputs(C, N, HW, center, regime, 'none', xs, backward=False)
    ref = SR.ln_reference(inp)
    bad = SR.ln_reference(inp, 'short_stats')
    for k in ('y', 'mu', 'rstd'):
        err = maxabs(SR.masked(bad[k], ref['live']), SR.masked(ref[k], ref['live']))
        assert err > ref['bar'][k], (k, err, ref['bar'][k])


@pytest.mark.parametrize('nparts,C', SR.PAIR_SUM_CASES)
def test_pair_sum_bar_can_fail(nparts, C):
    part = SR.pair_sum_inputs(nparts, C, 'random')
    ref, e32, b = SR.pair_sum_reference(part, nparts, C)
    if nparts == 1:
        assert ref.abs().max().item() > b           # dropping the only row leaves nothing
        return
    o0, o1, _ = SR.pair_sum_ref(part, torch.float64, drop_row=nparts - 1)
    assert maxabs(o0, ref[0]) > b and maxabs(o1, ref[1]) > b


@pytest.mark.parametrize('N,HW,xs', SR.CHANSUM_CASES)
def test_channel_sum_bar_can_fail(N, HW, xs):
    x = SR.channel_sum_inputs(N, HW, 'random')
    ref, e32, b = SR.channel_sum_reference(x)
    short = x.double().sum((0, 2, 3)) - x[-1, :, 0, -1].double()        # the last pixel of the last image left out
    assert (short - ref).abs().max().item() > b


@pytest.mark.parametrize('N,C,H,W', SR.DW_CASES)
def test_pooled_bar_can_fail(N, C, H, W):
    inp = SR.dw_inputs(N, C, H, W)
    g, pooled, mabs = SR.dw_ref(inp['t'], inp['w'], inp['b'], 'mul', torch.float64)
    e32 = maxabs(SR.dw_ref(inp['t'], inp['w'], inp['b'], 'mul', torch.float32)[1], pooled)
    b = SR.reduced_bar(e32, pooled, SR.pooled_depth(H, W), mabs)
    # one column block of one row (1024 of the H W pixels) left out of the mean
    short = (g.sum((2, 3)) - g[:, :, -1, :1024].sum(2)) / (H * W)
    assert (short - pooled).abs().max().item() > b
