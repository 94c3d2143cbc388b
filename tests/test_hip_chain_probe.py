"""Single-product probe of every GEMM stage of the fused NAFBlock chains (csrc/tdr_nafblock_chain.h and the four units that instantiate
it), with the builders of tests/_split_probe.py and the bars of DESIGN §4g: 2^-21 per element under bx3, 2^-20 under hx2.  The operands of
the inner stages are formed inside the kernels; they are steered from the outside instead of being fed directly:

    forward    conv1 (head), conv4 (tail)   the LayerNorm bias route: lnw = 0, lnb = v e_k -> the norm's output is v e_k at every pixel
               conv5 (tail)                 a zero tile makes t4 = b4; b4 non-zero at j and C + j -> the gate is one-hot at j
               conv3 (tail)                 g one-hot (tests/test_hip_split_probe.py::test_chain_conv3_stage)
    backward   conv5^T, conv3^T             dout one-hot, t4 = 1, lnw = 0 (dy = dout), beta = sca = 1: dt4 and dgp of one launch
               conv4^T (tail), conv1^T      K = 2C, every output row: one non-zero (channel, pixel) of the operand per workgroup, read
                                            off the workgroup's LayerNorm-gradient partial sum (its other 63 terms are exact zeros)
               the same two                 at every pixel: lnw = e_k turns row k of the GEMM into every other row of dy, times -1 / C
    twins      naf_*_infer, dyn_*_infer     bit-identical to the training kernels on the probe inputs; the text-modulated chains also with
                                            power-of-two modulation rows
               naf_tail_infer_local         gamma = 0 exposes y: its conv3 stage, and the channel-attention GEMM in front of it

Between the accumulator and the stored value there are only exact fp32 operations (+ 0, * 1, * 2^-k), so every bar is SP.BAR[cls] as it
stands; where two single products chain (the attention map of the TLSC tail feeding conv3) the bar is the sum of the two.  Operands that
are kernel products themselves (dt4, the gate) have one factor a power of two that keeps them in the fp16 window, and the test takes them
from the kernel's own stored tensor.  Under hx2 the backward chains run inside a loss-scaled pass (kernels.GRAD_SCALED), as in
tests/test_hip_nafblock_fused.py.  The float64 comparisons run on the device; every case prints `probe <kernel> <tag> <math>: max rel ...`."""
import pytest
import torch

import _split_probe as SP
from test_hip_split_probe import arithmetic, dev, sid

pytestmark = pytest.mark.gpu

CHAIN_MODES = ['bx3', 'hx2']
EPS = SP.CHAIN_EPS


class Tally:
    """the verdict of one case, kept on the device until the end: the worst relative error of the single products, and a count of
    everything that had to hold exactly and did not (non-zero outputs without a non-zero term, bitwise twins that differ)"""

    def __init__(self):
        self.worst = torch.zeros((), dtype=torch.float64, device='cuda')
        self.broken = torch.zeros((), dtype=torch.int64, device='cuda')

    def rel(self, out, exp, mask=None, zeros=True):
        """exp (float64) and mask broadcast against out; outside the mask the output must be exactly 0.0 unless zeros is False"""
        exp = exp.cuda() if not exp.is_cuda else exp
        assert torch.broadcast_shapes(out.shape, exp.shape) == out.shape, (tuple(out.shape), tuple(exp.shape))
        r = (out.double() - exp).abs() / exp.abs()
        if mask is not None:
            mask = mask.cuda() if not mask.is_cuda else mask
            if zeros:
                self.broken += ((out != 0) & ~mask).sum()
            r = torch.where(mask, r, torch.zeros((), dtype=torch.float64, device='cuda'))
        self.broken += torch.isnan(r).sum()
        self.worst = torch.maximum(self.worst, r.max())

    def same(self, a, b):
        """a == b element by element (a NaN counts as a difference)"""
        assert torch.broadcast_shapes(a.shape, b.shape) == a.shape, (tuple(a.shape), tuple(b.shape))
        self.broken += (a != b).sum()

    def holds(self, cond):
        self.broken += (~cond).sum()

    def window(self, op):
        """a kernel-formed operand lies in the fp16 window of SP.values"""
        self.holds((op.abs() >= SP.WINDOW[0]) & (op.abs() < SP.WINDOW[1]))

    def verdict(self, kernel, tag, math, cls, nbars=1):
        """prints the case's line; -> the list of what failed (empty: the case holds), for settle()"""
        worst, broken = self.worst.item(), self.broken.item()
        bar = nbars * SP.BAR[cls]
        print(f'probe {kernel} {tag} {math}: max rel {worst:.2e} (bar {bar:.2e})')
        failed = []
        if broken:
            failed.append(f'{kernel} {tag} {math}: {broken} elements that must hold exactly (zeros, bitwise twins, operand window) do not')
        if not 0 < worst <= bar:                                  # (0: nothing was compared; NaN fails as well)
            failed.append(f'{kernel} {tag} {math}: max rel {worst:.3e} against the bar {bar:.3e}')
        return failed


def settle(failed):
    """every stage of a case prints its line before the case fails for any of them"""
    assert not failed, '; '.join(failed)


def _pack(K, w, mode):
    return K.pack_weights(dev(w), mode)[0]


def _rows(N, width, a, b):
    return torch.full((N, width), a, device='cuda'), torch.full((N, width), b, device='cuda')


def _couts(C):
    return [C] + ([C // 2] if C >= 64 else [])                # c_out = C / 2 must be a multiple of 32 (kernels.naf_tail_supported)


# ------------------------------------------------------------------ forward chains
@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_head_conv1_stage(mode, shape):
    """naf_head_fwd by the bias route, one K index per launch, all C of them: the stored xn is lnb bitwise and t1[o, p] = W1[o, k] v.
    naf_head_infer and dyn_head_infer (rows a = 1, b = 0) give the same bits; dyn_head_infer with power-of-two rows -- which change the
    LayerNorm input and nothing behind a zero LayerNorm weight -- is held to the same bar."""
    N, C, H, W = shape
    V = []
    with arithmetic(mode) as K:
        assert K.naf_tail_supported(C, H * W)
        i0, _, _ = SP.build_head_conv1(N, C, H, W, 0)
        x, lnw, b1, w1p = dev(i0['x']), dev(i0['lnw']), dev(i0['b1']), _pack(K, i0['w1'], K.PACK_FWD)
        one, zero = _rows(N, C, 1.0, 0.0)
        ma, mb = (dev(t) for t in SP.mod_rows(N, C))
        keep, dyn = Tally(), Tally()
        for k in range(C):
            inp, exp, _ = SP.build_head_conv1(N, C, H, W, k)
            lnb, exp = dev(inp['lnb']), exp.cuda()
            xn, mu, rs, t1 = K.naf_head_fwd(x, lnw, lnb, EPS, w1p, b1)
            assert t1.shape == (N, 2 * C, H, W)
            keep.same(xn, lnb.view(1, C, 1, 1))
            keep.rel(t1, exp)
            keep.same(K.naf_head_infer(x, lnw, lnb, EPS, w1p, b1), t1)
            dyn.same(K.dyn_head_infer(x, one, zero, lnw, lnb, EPS, w1p, b1), t1)
            dyn.rel(K.dyn_head_infer(x, ma, mb, lnw, lnb, EPS, w1p, b1), exp)
        V += keep.verdict('naf_head_fwd_conv1', sid(shape), mode, mode)
        V += dyn.verdict('dyn_head_infer_conv1', sid(shape), mode, mode)
    settle(V)


@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_tail_conv4_stage(mode, shape):
    """naf_tail_fwd by the bias route on norm2, all C K indices: y = x and yn = lnb bitwise, t4[o, p] = W4[o, k] v on all 2C rows;
    naf_tail_infer and dyn_tail_infer (a = 1, b = 0) give the bits of `out`"""
    N, C, H, W = shape
    V = []
    with arithmetic(mode) as K:
        i0, _, _ = SP.build_tail_conv4(N, C, H, W, 0)
        d = {k: dev(v) for k, v in i0.items() if k not in ('w3', 'w4', 'w5', 'lnb')}
        w3p, w4p, w5p = (_pack(K, i0[k], K.PACK_FWD) for k in ('w3', 'w4', 'w5'))
        one, zero = _rows(N, 2 * C, 1.0, 0.0)
        t = Tally()
        for k in range(C):
            inp, exp, _ = SP.build_tail_conv4(N, C, H, W, k)
            lnb = dev(inp['lnb'])
            args = (d['g'], d['sca'], d['x'], w3p, d['b3'], d['beta'], d['lnw'], lnb, EPS, w4p, d['b4'])
            out, y, mu, rs, yn, t4 = K.naf_tail_fwd(*args, w5p, d['b5'], d['gamma'])
            assert t4.shape == (N, 2 * C, H, W)
            t.same(y, d['x'])
            t.same(yn, lnb.view(1, C, 1, 1))
            t.rel(t4, exp)
            t.holds(torch.isfinite(out))
            t.same(K.naf_tail_infer(*args, w5p, d['b5'], d['gamma']), out)
            t.same(K.dyn_tail_infer(*args, one, zero, w5p, d['b5'], d['gamma']), out)
        V += t.verdict('naf_tail_fwd_conv4', sid(shape), mode, mode)
    settle(V)


@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_tail_conv5_stage(mode, shape):
    """naf_tail_fwd with t4 = b4 (a zero tile), all C K indices, c_out = C and C / 2: the stored t4 is b4 bitwise, the gate operand
    fl32(t4[j] t4[C + j]) -- taken from the stored t4 -- is the builder's, and out[o, p] = W5[o, j] operand.  naf_tail_infer and
    dyn_tail_infer (a = 1, b = 0) give the same bits; dyn_tail_infer with power-of-two rows (t4 = fma(0, a, fma(b4, a, b)), exact) is held to
    the same bar."""
    N, C, H, W = shape
    V = []
    with arithmetic(mode) as K:
        i0, _, _ = SP.build_tail_conv5(N, C, H, W, 0)
        d = {k: dev(v) for k, v in i0.items() if k in ('g', 'sca', 'x', 'b3', 'beta', 'lnw', 'lnb', 'b5', 'gamma')}
        w3p, w4p = _pack(K, i0['w3'], K.PACK_FWD), _pack(K, i0['w4'], K.PACK_FWD)
        w5 = dev(i0['w5'])
        w5d = w5.view(C, C).double()
        w5p = {co: _pack(K, i0['w5'][:co].contiguous(), K.PACK_FWD) for co in _couts(C)}
        one, zero = _rows(N, 2 * C, 1.0, 0.0)
        im = SP.build_tail_conv5(N, C, H, W, 0, mod=True)[0]
        ma, mb = dev(im['a2']), dev(im['b2'])
        keep, dyn = {co: Tally() for co in _couts(C)}, Tally()
        for j in range(C):
            inp, _, _ = SP.build_tail_conv5(N, C, H, W, j)
            b4 = dev(inp['b4'])
            head = (d['g'], d['sca'], d['x'], w3p, d['b3'], d['beta'], d['lnw'], d['lnb'], EPS, w4p, b4)
            for co in _couts(C):
                t = keep[co]
                out, y, mu, rs, yn, t4 = K.naf_tail_fwd(*head, w5p[co], d['b5'], d['gamma'], c_out=co)
                assert out.shape == (N, co, H, W)
                t.same(t4, dev(inp['t4']).view(N, 2 * C, 1, 1))
                op = t4[:, j] * t4[:, C + j]
                t.same(op, dev(inp['operand']).view(N, 1, 1))
                t.window(op)
                t.rel(out, w5d[:co, j].view(1, co, 1, 1) * op.double()[:, None])
                t.same(K.naf_tail_infer(*head, w5p[co], d['b5'], d['gamma'], c_out=co), out)
                if co == C:
                    dyn.same(K.dyn_tail_infer(*head, one, zero, w5p[C], d['b5'], d['gamma']), out)
            inp, exp, _ = SP.build_tail_conv5(N, C, H, W, j, mod=True)
            head = head[:-1] + (dev(inp['b4']),)
            dyn.rel(K.dyn_tail_infer(*head, ma, mb, w5p[C], d['b5'], d['gamma']), exp)
        for co in _couts(C):
            V += keep[co].verdict('naf_tail_fwd_conv5', f'{sid(shape)} c_out={co}', mode, mode)
        V += dyn.verdict('dyn_tail_infer_conv5', sid(shape), mode, mode)
    settle(V)


@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_tail_conv3_stage_twins(mode, shape):
    """the forward-only twins on the inputs of test_hip_split_probe.py::test_chain_conv3_stage with plain LayerNorm / conv4 / conv5
    parameters: naf_tail_infer and dyn_tail_infer (a = 1, b = 0) give the bits of naf_tail_fwd's `out`"""
    N, C, H, W = shape
    (g, w3), _, _ = SP.build_conv(N, C, C, H, W, 1, seed=3)
    wts = SP.chain_weights(C)
    with arithmetic(mode) as K:
        w3p, w4p, w5p = (_pack(K, w * s, K.PACK_FWD) for w, s in ((w3, 1.0), (wts['w4'], C ** -0.5 / 2), (wts['w5'], C ** -0.5 / 2)))
        v = lambda n, seed: dev(SP.values(n, seed=seed)) * 0.25
        args = (dev(g), torch.ones(N, C, device='cuda'), torch.zeros(N, C, H, W, device='cuda'), w3p, torch.zeros(C, device='cuda'),
                torch.ones(C, device='cuda'), v(C, 1), v(C, 2), EPS, w4p, v(2 * C, 3))
        one, zero = _rows(N, 2 * C, 1.0, 0.0)
        out, *_ = K.naf_tail_fwd(*args, w5p, v(C, 4), v(C, 5))
        t = Tally()
        t.holds(torch.isfinite(out))
        t.same(K.naf_tail_infer(*args, w5p, v(C, 4), v(C, 5)), out)
        t.same(K.dyn_tail_infer(*args, one, zero, w5p, v(C, 4), v(C, 5)), out)
        assert t.broken.item() == 0


# ------------------------------------------------------------------ backward chains
@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_tail_bwd_conv5t_and_conv3t(mode, shape):
    """one launch of naf_tail_bwd per c_out: both halves of dt4 are W5[o(p), c] dout[o(p), p] (K = c_out), dy is dout bitwise on the first
    c_out rows and exact zeros above, dgp[c, p] = W3[o(p), c] dout[o(p), p]"""
    N, C, H, W = shape
    V = []
    with arithmetic(mode, grad_scaled=mode == 'hx2') as K:
        for co in _couts(C):
            inp, exp = SP.build_tail_bwd_conv53(N, C, H, W, co)
            d = {k: dev(v) for k, v in inp.items() if not k.startswith('w')}
            w5t, w4t, w3t = (_pack(K, inp[k], K.PACK_DGRAD_S1) for k in ('w5', 'w4', 'w3'))
            dy, dt4, gw, gb, dgp = K.naf_tail_bwd(d['dout'], d['gamma'], d['t4'], d['y'], d['mu'], d['rs'], d['lnw'], w5t, w4t, w3tp=w3t,
                                                  beta=d['beta'], sca=d['sca'])
            assert dt4.shape == (N, 2 * C, H, W) and dy.shape == dgp.shape == (N, C, H, W)
            t5, t3 = Tally(), Tally()
            t5.rel(dt4, *exp['dt4'])
            t3.same(dy, exp['dy'][0].float().cuda())
            t3.rel(dgp, *exp['dgp'])
            V += t5.verdict('naf_tail_bwd_conv5T', f'{sid(shape)} c_out={co}', mode, mode)
            V += t3.verdict('naf_tail_bwd_conv3T', f'{sid(shape)} c_out={co}', mode, mode)
    settle(V)


def _partials(fin, nparts, C):
    """the raw per-workgroup partials of a deferred launch: [workgroup][gw: C | gb: C] -> (gw, gb), each [workgroups, C]"""
    assert fin.dims == (nparts, C)
    p = fin.ws[:nparts * 2 * C].view(nparts, 2, C)
    return p[:, 0], p[:, 1]


@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_head_bwd_conv1t_every_row(mode, shape):
    """naf_head_bwd, sixteen launches: the gb partial row of every workgroup is W1[j, c] dt1[j, p*] for all C rows c, j reaching all 2C K
    indices and p* all 64 pixel slots; the gw partials are exact zeros (yhat = 0) and dx is res bitwise (lnw = 0).  One more launch with
    yhat = 1: the gw partials are the gb partials bitwise."""
    N, C, H, W = shape
    V = []
    nparts = N * (H * W // 64)
    with arithmetic(mode, grad_scaled=mode == 'hx2') as K:
        w1t = _pack(K, SP.chain_weights(C)['w1'], K.PACK_DGRAD_S1)
        t = Tally()
        for launch, yhat in [(l, 0) for l in range(SP.PARTIAL_LAUNCHES)] + [(0, 1)]:
            inp, exp, _ = SP.build_head_bwd_partials(N, C, H, W, launch, yhat)
            d = {k: dev(v) for k, v in inp.items() if k != 'w1'}
            dx, fin, _ = K.naf_head_bwd(d['dt1'], d['x'], d['mu'], d['rs'], d['lnw'], w1t, d['res'], defer_finish=True)
            gw, gb = _partials(fin, nparts, C)
            t.rel(gb, exp)
            t.same(gw, gb if yhat else torch.zeros_like(gb))
            t.same(dx, d['res'])
        V += t.verdict('naf_head_bwd_conv1T_partials', sid(shape), mode, mode)
    settle(V)


@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_tail_bwd_conv4t_every_row(mode, shape):
    """naf_tail_bwd, sixteen launches: the stored dt4 is non-zero only at ((j + C) mod 2C, p*) of each workgroup, a single product of conv5^T
    times a power of two, inside the window; the gb partial row of the workgroup is W4[(j + C) mod 2C, c] times that stored value for all C
    rows; gw partials zero, dy = dout bitwise.  One more launch with yhat = 1: gw partials = gb partials bitwise."""
    N, C, H, W = shape
    V = []
    nparts = N * (H * W // 64)
    with arithmetic(mode, grad_scaled=mode == 'hx2') as K:
        wts = SP.chain_weights(C)
        w5t, w4t = _pack(K, wts['w5'], K.PACK_DGRAD_S1), _pack(K, wts['w4'], K.PACK_DGRAD_S1)
        t5, t4_ = Tally(), Tally()
        for launch, yhat in [(l, 0) for l in range(SP.PARTIAL_LAUNCHES)] + [(0, 1)]:
            inp, (n, jp, p), (edt4, mdt4), w4rows = SP.build_tail_bwd_partials(N, C, H, W, launch, yhat)
            d = {k: dev(v) for k, v in inp.items() if not k.startswith('w')}
            dy, dt4, fin, _ = K.naf_tail_bwd(d['dout'], d['gamma'], d['t4'], d['y'], d['mu'], d['rs'], d['lnw'], w5t, w4t, defer_finish=True)
            gw, gb = _partials(fin, nparts, C)
            t5.rel(dt4, edt4, mdt4)
            op = dt4.view(N, 2 * C, H * W)[n.cuda(), jp.cuda(), p.cuda()]
            t4_.window(op)
            t4_.rel(gb, w4rows.cuda() * op.double()[:, None])
            t4_.same(gw, gb if yhat else torch.zeros_like(gb))
            t4_.same(dy, d['dout'])
        V += t5.verdict('naf_tail_bwd_conv5T_sparse_gate', sid(shape), mode, mode)
        V += t4_.verdict('naf_tail_bwd_conv4T_partials', sid(shape), mode, mode)
    settle(V)


def _rows_agree(t, dy, mask):
    """all rows of dy inside the mask carry the same bits at every pixel"""
    mask = mask.cuda()
    inf = torch.full((), float('inf'), device='cuda')
    hi = torch.where(mask, dy, -inf).amax(1)
    lo = torch.where(mask, dy, inf).amin(1)
    t.same(hi, lo)


@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_head_bwd_conv1t_every_pixel(mode, shape):
    """naf_head_bwd with lnw = e_k, one k per wave: every row c != k of dx is -W1[j(p), k] dt1[j(p), p] / C at every pixel, all those rows
    with the same bits (both K halves of the three-plane kernel at every pixel slot)"""
    N, C, H, W = shape
    V = []
    with arithmetic(mode, grad_scaled=mode == 'hx2') as K:
        w1t = _pack(K, SP.chain_weights(C)['w1'], K.PACK_DGRAD_S1)
        t = Tally()
        for k in SP.dy_route_rows(C):
            inp, exp, mask = SP.build_head_bwd_dy(N, C, H, W, k)
            d = {kk: dev(v) for kk, v in inp.items() if kk != 'w1'}
            dx, gw, gb = K.naf_head_bwd(d['dt1'], d['x'], d['mu'], d['rs'], d['lnw'], w1t, d['res'])
            assert dx.shape == (N, C, H, W)
            t.rel(dx, exp, mask, zeros=False)
            _rows_agree(t, dx, mask)
        V += t.verdict('naf_head_bwd_conv1T_dx', sid(shape), mode, mode)
    settle(V)


@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_tail_bwd_conv4t_every_pixel(mode, shape):
    """naf_tail_bwd with lnw = e_k, one k per wave, dt4 one-hot at every pixel (the stored dt4: a single product of conv5^T times a power of
    two, inside the window): every row of dy outside {k, o(p)} is -W4[j'(p), k] dt4[j'(p), p] / C, all with the same bits"""
    N, C, H, W = shape
    V = []
    with arithmetic(mode, grad_scaled=mode == 'hx2') as K:
        wts = SP.chain_weights(C)
        w5t, w4t = _pack(K, wts['w5'], K.PACK_DGRAD_S1), _pack(K, wts['w4'], K.PACK_DGRAD_S1)
        t5, t4_ = Tally(), Tally()
        for k in SP.dy_route_rows(C):
            inp, (n, jp, p), (edt4, mdt4), w4col, mask = SP.build_tail_bwd_dy(N, C, H, W, k)
            d = {kk: dev(v) for kk, v in inp.items() if not kk.startswith('w')}
            dy, dt4, gw, gb = K.naf_tail_bwd(d['dout'], d['gamma'], d['t4'], d['y'], d['mu'], d['rs'], d['lnw'], w5t, w4t)
            t5.rel(dt4, edt4, mdt4)
            op = dt4.view(N, 2 * C, H * W)[n.cuda(), jp.cuda(), p.cuda()].view(N, 1, H, W)
            t4_.window(op)
            t4_.rel(dy, -w4col.cuda() * op.double() / C, mask, zeros=False)
            _rows_agree(t4_, dy, mask)
        V += t5.verdict('naf_tail_bwd_conv5T_onehot_gate', sid(shape), mode, mode)
        V += t4_.verdict('naf_tail_bwd_conv4T_dy', sid(shape), mode, mode)
    settle(V)


# ------------------------------------------------------------------ the TLSC tail
@pytest.mark.parametrize('shape', SP.CHAIN_SHAPES, ids=sid)
@pytest.mark.parametrize('mode', CHAIN_MODES)
def test_local_tail_conv3_and_attention_stages(mode, shape):
    """naf_tail_infer_local with gamma = 0 (out = y).  conv3: attention map 1.0 (pooled = 0, bsca = 1), g one-hot.  wsca: pooled one-hot,
    g = 1.0 at one channel per pixel -- conv3's operand there is the single product of the attention GEMM, so y is two single products in
    a chain and its bar is twice the bar of one."""
    N, C, H, W = shape
    V = []
    cases = SP.build_local_stages(N, C, H, W)
    with arithmetic(mode) as K:
        for stage, nbars in (('conv3', 1), ('wsca', 2)):
            inp, exp, mask = cases[stage]
            d = {k: dev(v) for k, v in inp.items() if not k.startswith('w')}
            wscap, w3p, w4p, w5p = (_pack(K, inp[k], K.PACK_FWD) for k in ('wsca', 'w3', 'w4', 'w5'))
            out = K.naf_tail_infer_local(d['g'], d['pooled'], d['x'], wscap, d['bsca'], w3p, d['b3'], d['beta'], d['lnw'], d['lnb'], EPS, w4p,
                                         d['b4'], w5p, d['b5'], d['gamma'])
            t = Tally()
            t.rel(out, exp, mask)
            V += t.verdict(f'naf_tail_infer_local_{stage}', sid(shape), mode, mode, nbars)
    settle(V)
