"""The streaming kernels of csrc/tdr_pointwise.hip (LayerNorm2d forward / backward, the SCA chain, tdr_pair_sum_partials, channel_sum,
copy_rows / add_rows) and the depthwise-gate forward stencils of csrc/tdr_dwsg.hip past one column block, against the float64
references of tests/_stream_ref.py, at the smallest shapes that reach each dispatch branch.  No convolution is launched: the arithmetic
mode does not matter and `kernels` is taken as it comes.

Branches and the cases that reach them (ids as pytest prints them; profiles/stream_float64/README.md has the full map):
    LayerNorm forward    _stream_ref.LN_FWD_CASES (C, N, HW, center, regime, x sliced): both ends of every C bracket of ln_fwd_kernel,
                         ln_fwd_narrow_kernel<12 / 24>, ln_fwd_generic_kernel by C > 1536 and by N ceil(HW / 64) = 512 (511 stays narrow)
    LayerNorm backward   _stream_ref.LN_BWD_CASES (..., add, x sliced, add sliced): ln_bwd_kernel with one and with two trips of its
                         256-block grid, ln_bwd_cached_kernel<16 / 32>, ln_bwd_generic_kernel<true>, and <false> + ln_param_grad_kernel
                         at 1029 tiles; every branch with both center values, add absent / full / add_C < C, x as a channel slice with N >= 2
    regimes              randn | a per-pixel offset of 50 sigma with every seventh channel 8 times as wide | two zero-variance pixels
    SCA chain            C in 6 .. 512 (the ci += 256 trip, colb = 2, the co >= C tail, ragged 64-wide tiles), N in 1, 3; Cout != Cin
    finishers            tdr_pair_sum_partials one-stage and two-stage (slice layout 2C < 256, 2C = 96 and 140 included; column layout 2C >= 256)
    rows                 the float4 path, the three ways into the scalar path, one grid-striding length each
    stencils             dwsg_fwd (+ pooled), dwgelu_fwd, dwconv_fwd at W = 1028 (2 column blocks) and W = 2052 (3)

Bars: none is typed in and none comes from the kernel.  Element-wise outputs: e32 = max |float32 run - float64 run| of the reference,
bar = max(8 e32, 4 float32 ulp of max |ref64|) (_masa_ref.bar).  Outputs summed over pixels or partial rows (gw, gb, channel_sum,
pair_sum_partials, pooled): the larger of that and depth 2^-24 max_c sum |t_i|, depth counted in the kernel's loops
(_stream_ref.*_depth).  Pure sums and moves on integer-valued inputs: equality with float64.  The dead pixels (rstd = 1 / sqrt(eps))
are compared apart from the others, against their own e32 and bar.  Every case prints kernel error, e32 and bar; the captured output
is kept as profiles/stream_float64/test_hip_stream_float64.log.  Measured on the MI355X: every element-wise output at or below 0.22
of its bar (mu of ln_fwd_kernel<16,32> and ln_fwd_narrow_kernel<24>), gx at or below 0.17, gw / gb and the finishers at 0.001 - 0.15;
every integer-regime sum and every row copy equal to float64.  (gx of ln_bwd_generic_kernel<true> at C = 1024 under the 50 sigma offset
reached 0.61 when the backward ran on the forward kernel's own mu / rstd: the forward's error carried through.)"""
import pytest
import torch

import _stream_ref as SR
from _masa_ref import bar, maxabs

pytestmark = pytest.mark.gpu

HUGE = 1e30            # fills the channels around a channel slice: a read outside the slice swamps every output

_cache = {}


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels
    return kernels


def ident(case):
    return '-'.join(str(v) for v in case)


def cached(key, build):
    """references are built once per case and shared by the tests of that case (never modified)"""
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def line(what, err, e32, b):
    print(f'{what}: kernel {err:.3e}  e32 {e32:.3e}  bar {b:.3e}')
    return err <= b


def channel_slice(t, fill=HUGE):
    """t [N, C, H, W] as channels PAD_LO .. PAD_LO + C of a wider device tensor"""
    N, C, H, W = t.shape
    wide = torch.full((N, SR.PAD_LO + C + SR.PAD_HI, H, W), fill, device='cuda')
    wide[:, SR.PAD_LO:SR.PAD_LO + C] = t.cuda()
    return wide[:, SR.PAD_LO:SR.PAD_LO + C]


# ------------------------------------------------------------------------------------------------------------------ LayerNorm2d
def ln_case(case, backward):
    def build():
        inp = SR.ln_inputs(*case, backward=True) if backward else SR.ln_inputs(*case[:5], 'none', case[5], backward=False)
        return inp, SR.ln_reference(inp)
    return cached(('ln', backward) + tuple(case), build)


def ln_run(K, inp, go=None, ref=None):
    """layernorm2d_fwd, and where go is given layernorm2d_bwd on the float64 reference's mu / rstd rounded to float32: the forward
    kernel's own error (held to its bar by the same case) can neither hide nor add to an error of the backward kernel"""
    x = channel_slice(inp['x']) if inp['xs'] else inp['x'].cuda()
    w = inp['w'].cuda()
    b = inp['b'].cuda() if inp['b'] is not None else None
    y, mu, rstd = K.layernorm2d_fwd(x, w, b, SR.EPS, center=bool(inp['center']))
    got = dict(y=y, mu=mu, rstd=rstd)
    if go is not None:
        add = None
        if inp['add_wide'] is not None:
            wide = inp['add_wide'].cuda()
            add = wide[:, inp['add_lo']:inp['add_lo'] + inp['add_C']]
        gx, gw, gb = K.layernorm2d_bwd(go.cuda(), x, ref['mu'].float().cuda(), ref['rstd'].float().cuda(), w, add=add,
                                       center=bool(inp['center']))
        got.update(gx=gx, gw=gw, gb=gb)
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in got.items()}


def ln_check(tag, inp, ref, got, keys):
    m, fails = ref['live'], []
    for k in keys:
        if k in ('gw', 'gb'):
            ok = line(f'{tag} {k}', maxabs(got[k], ref[k]), ref['e32'][k], ref['bar'][k])
        else:
            ok = line(f'{tag} {k}', maxabs(SR.masked(got[k], m), SR.masked(ref[k], m)), ref['e32'][k], ref['bar'][k])
            if inp['dead']:
                ok &= line(f'{tag} {k} (dead pixels)', maxabs(SR.masked(got[k], 1 - m), SR.masked(ref[k], 1 - m)), ref['e32_dead'][k],
                           ref['bar_dead'][k])
            assert torch.isfinite(got[k]).all()
        if not ok:
            fails.append(k)
    for n, p, v in inp['dead']:
        # a zero-variance pixel: the mean is exact, so y is the bias alone (BiasFree: x rstd w, which is 0 at the pixel of value 0)
        assert (got['mu'][n, p] == v).all()
        if inp['center']:
            assert torch.equal(got['y'][n, :, 0, p], inp['b'])
        elif v == 0:
            assert (got['y'][n, :, 0, p] == 0).all()
    assert not fails, fails


@pytest.mark.parametrize('case', SR.LN_FWD_CASES, ids=ident)
def test_layernorm2d_fwd(K, case):
    inp, ref = ln_case(case, False)
    ln_check(f'ln_fwd {ident(case)} [{SR.ln_fwd_kernel_name(*case[:3])}]', inp, ref, ln_run(K, inp), SR.LN_FORWARD)


@pytest.mark.parametrize('case', SR.LN_BWD_CASES, ids=ident)
def test_layernorm2d_bwd(K, case):
    inp, ref = ln_case(case, True)
    got = ln_run(K, inp, inp['go'], ref)
    ln_check(f'ln_bwd {ident(case)} [{SR.ln_bwd_kernel_name(*case[:3])}]', inp, ref, got, SR.LN_ELEMENTWISE + ('gw', 'gb'))


@pytest.mark.parametrize('case', SR.LN_BWD_EXACT_GB, ids=ident)
def test_layernorm2d_bwd_gb_exact(K, case):
    """integer-valued go: gb = sum go is exact in float32 in any order"""
    inp, ref = ln_case(case, True)
    go = SR.int_values(inp['go'].shape, SR._gen(SR.case_seed('gb', *case)))
    got = ln_run(K, inp, go, ref)
    want = go.double().sum((0, 2, 3))
    print(f'ln_bwd {ident(case)} [{SR.ln_bwd_kernel_name(*case[:3])}] gb on integer go: max |kernel - float64| '
          f'{maxabs(got["gb"], want):.3e} (equality asked)')
    assert torch.equal(got['gb'].double(), want)


# ------------------------------------------------------------------------------------------------------------------ SCA chain
@pytest.mark.parametrize('C,N,regime', SR.SCA_CASES)
def test_sca_chain(K, C, N, regime):
    inp = SR.sca_inputs(C, N, regime)
    ref = SR.sca_reference(inp)
    G3, S3, pooled = (inp[k].float().cuda() for k in ('G3', 'S3', 'pooled'))
    w3, b3, beta, wsca, bsca = (inp[k].cuda() for k in ('w3', 'b3', 'beta', 'wsca', 'bsca'))
    s = K.sca_fwd(pooled, wsca, bsca)
    out = K.sca_bwd(G3, S3, w3, b3, beta, s, pooled, wsca)
    torch.cuda.synchronize()
    got = dict(zip(SR.SCA_OUT, (s,) + tuple(out)))
    fails = [k for k in SR.SCA_OUT
             if not line(f'sca C={C} N={N} {regime} {k}', maxabs(got[k].cpu().reshape(ref[k].shape), ref[k]), ref['e32'][k], ref['bar'][k])]
    assert not fails, fails
    if regime == 'integer':
        assert torch.equal(got['dbsca'].cpu().double(), ref['dbsca'])


@pytest.mark.parametrize('Cout,Cin,extra', SR.PARAM_CASES)
def test_scaled_conv_param_grads(K, Cout, Cin, extra):
    """the gamma chain, Cout != Cin; extra > 0: w / b / gamma hold more rows than Cout"""
    inp = SR.param_inputs(Cout, Cin, extra)
    ref = SR.param_reference(inp)
    dw, db, dg = K.scaled_conv_param_grads(inp['G'].float().cuda(), inp['S'].float().cuda(), inp['w'].cuda(), inp['b'].cuda(),
                                           inp['gamma'].cuda())
    torch.cuda.synchronize()
    got = dict(dw=dw, db=db, dgamma=dg)
    fails = [k for k in got
             if not line(f'param Cout={Cout} Cin={Cin} {k}', maxabs(got[k].cpu().reshape(ref[k].shape), ref[k]), ref['e32'][k], ref['bar'][k])]
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------------ plain sums
@pytest.mark.parametrize('regime', SR.REGIMES)
@pytest.mark.parametrize('nparts,C', SR.PAIR_SUM_CASES)
def test_pair_sum_partials(K, nparts, C, regime):
    lib = __import__('textualdegremoval_amd._lib', fromlist=['load']).load()
    part = SR.pair_sum_inputs(nparts, C, regime)
    ref, e32, b = SR.pair_sum_reference(part, nparts, C)
    nmid = int(lib.tdr_pair_sum_mid_floats(nparts, C))
    assert nmid == (SR.cdiv(nparts, 256) * 2 * C if nparts > 1024 else 0)
    mid = torch.full((max(nmid, 1),), float('nan'), device='cuda')
    o = torch.full((2, C), float('nan'), device='cuda')
    pd = part.cuda()
    K.check(lib.tdr_pair_sum_partials(pd.data_ptr(), nparts, C, o[0].data_ptr(), o[1].data_ptr(), mid.data_ptr() if nmid else 0,
                                      K._stream()), 'tdr_pair_sum_partials')
    torch.cuda.synchronize()
    err = maxabs(o.cpu(), ref)
    ok = line(f'pair_sum nparts={nparts} C={C} {regime} [{"two-stage" if nparts > 1024 else "one-stage"}]', err, e32, b)
    if regime == 'integer':
        assert torch.equal(o.cpu().double(), ref)
    assert ok


@pytest.mark.parametrize('regime', SR.REGIMES)
@pytest.mark.parametrize('N,HW,xs', SR.CHANSUM_CASES)
def test_channel_sum(K, N, HW, xs, regime):
    x = SR.channel_sum_inputs(N, HW, regime)
    ref, e32, b = SR.channel_sum_reference(x)
    got = K.channel_sum(channel_slice(x) if xs else x.cuda()).cpu()
    ok = line(f'channel_sum N={N} HW={HW} sliced={xs} {regime}', maxabs(got, ref), e32, b)
    if regime == 'integer':
        assert torch.equal(got.double(), ref)
    assert ok


@pytest.mark.parametrize('add', [False, True], ids=['copy_rows', 'add_rows'])
@pytest.mark.parametrize('case', SR.ROWS_CASES, ids=lambda c: c[0])
def test_rows(K, case, add):
    name, N, length, src_ns, dst_ns, off = case
    src, dst = SR.rows_inputs(*case)
    want = SR.rows_ref(src, dst, N, length, src_ns, dst_ns, off, add)
    s, d = src.cuda(), dst.cuda()
    sv = s[off:]
    assert (SR.rows_path(N, length, src_ns, dst_ns, off) == 'rows_kernel') == (sv.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
                                                                                and length % 4 == 0 and src_ns % 4 == 0 and dst_ns % 4 == 0)
    (K.add_rows if add else K.copy_rows)(sv, src_ns, d, dst_ns, N, length)
    torch.cuda.synchronize()
    err = maxabs(d.cpu(), want)
    print(f'{"add_rows" if add else "copy_rows"} {name} [{SR.rows_path(N, length, src_ns, dst_ns, off)}]: max |kernel - float64| {err:.3e} '
          '(equality asked, the gaps between the rows included)')
    assert torch.equal(d.cpu().double(), want)
    assert torch.equal(s.cpu(), src)


# ------------------------------------------------------------------------------------------------- depthwise-gate forward stencils
def dw_case(N, C, H, W, gate):
    def build():
        inp = SR.dw_inputs(N, C, H, W)
        return inp, SR.dw_ref(inp['t'], inp['w'], inp['b'], gate, torch.float64), SR.dw_ref(inp['t'], inp['w'], inp['b'], gate, torch.float32)
    return cached(('dw', N, C, H, W, gate), build)


@pytest.mark.parametrize('N,C,H,W', SR.DW_CASES)
def test_dwsg_fwd_wide(K, N, C, H, W):
    inp, (g64, p64, mabs), (g32, p32, _) = dw_case(N, C, H, W, 'mul')
    g, pooled = K.dwsg_fwd(inp['t'].cuda(), inp['w'].cuda(), inp['b'].cuda())
    e32 = maxabs(g32, g64)
    ok = line(f'dwsg_fwd {N}x{C}x{H}x{W} g', maxabs(g.cpu(), g64), e32, bar(e32, g64))
    e32 = maxabs(p32, p64)
    ok &= line(f'dwsg_fwd {N}x{C}x{H}x{W} pooled', maxabs(pooled.cpu(), p64), e32, SR.reduced_bar(e32, p64, SR.pooled_depth(H, W), mabs))
    assert ok


@pytest.mark.parametrize('N,C,H,W', SR.DW_CASES)
def test_dwgelu_fwd_wide(K, N, C, H, W):
    inp, g64, g32 = dw_case(N, C, H, W, 'gelu')
    g = K.dwgelu_fwd(inp['t'].cuda(), inp['w'].cuda(), inp['b'].cuda())
    e32 = maxabs(g32, g64)
    assert line(f'dwgelu_fwd {N}x{C}x{H}x{W} g', maxabs(g.cpu(), g64), e32, bar(e32, g64))


@pytest.mark.parametrize('N,C,H,W', SR.DW_CASES)
def test_dwconv_fwd_wide(K, N, C, H, W):
    inp, u64, u32 = dw_case(N, C, H, W, 'none')
    u = K.dwconv_fwd(inp['t'].cuda(), inp['w'].cuda(), inp['b'].cuda())
    e32 = maxabs(u32, u64)
    assert line(f'dwconv_fwd {N}x{C}x{H}x{W} out', maxabs(u.cpu(), u64), e32, bar(e32, u64))
