"""tdr_freq_loss on the GPU (csrc/tdr_freq_loss.hip) through kernels.freq_loss and losses.FFTLoss, against the float64 reference of
tests/_freq_loss_ref.py by the rule of tests/test_hip_masa_kernels.py: spectrum, value and dpred each within max(8 x the error of the
same reference run in float32, 4 float32 ulp of the reference's magnitude); no bar is typed in.  The case table guarantees that no bin
lies within 16 x the float32 reference's spectrum error of zero, so the signs -- and with them the gradient -- are compared straight.

Measured on an MI355X (profiles/freq_loss/errors.txt holds the printed lines of all 24 runs): the spectrum is 0.61 - 1.15 x s32 from float64,
dpred 0.64 - 1.83 x e32 (exact at 4 x 4, two-sided), the value at most 0.14 of its bar; every sign equal."""
import numpy as np
import pytest
import torch

import _freq_loss_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels
    return kernels


_dev = {}


def _device_run(K, run):
    """inputs on the device and ONE kernel run per (case, mode), shared read-only by the tests"""
    if run not in _dev:
        case, onesided = run
        ref = R.reference(case, onesided)
        pred, gt = ref['pred'].cuda(), ref['gt'].cuda()
        loss, dpred, spec = K.freq_loss(pred, gt, case[2], onesided, want_spectrum=True)
        _dev[run] = dict(pred=pred, gt=gt, loss=loss, dpred=dpred, spec=spec)
    return _dev[run]


@pytest.mark.parametrize('run', R.RUNS, ids=R.run_id)
def test_against_float64(K, run):
    case, onesided = run
    d, ref = _device_run(K, run), R.reference(case, onesided)
    spec, dpred = d['spec'].cpu(), d['dpred'].cpu()
    s_err, s_bar = R.maxabs(spec, ref['spec64']), R.bar(ref['s32'], ref['spec64'])
    v_err, v_bar = abs(float(d['loss'].item()) - ref['loss64']), R.ulp_bar(ref['v32'], ref['loss64'])
    g_err, g_bar = R.maxabs(dpred, ref['dpred64']), R.bar(ref['e32'], ref['dpred64'])
    top = ref['dpred64'].abs().max().item()
    H, W = case[0][2:]
    print(f'{R.run_id(run)}: spec err {s_err:.3e} s32 {ref["s32"]:.3e} bar {s_bar:.3e} mgn {ref["mgn"]:.3e} | '
          f'loss err {v_err:.2e} v32 {ref["v32"]:.2e} bar {v_bar:.2e} | dpred err {g_err:.3e} e32 {ref["e32"]:.3e} bar {g_bar:.3e} '
          f'max|dpred64| {top:.3e} | max|dpred| numel / (w sqrt(HW)) {top * dpred.numel() / (case[2] * (H * W) ** 0.5):.2f}')
    assert torch.isfinite(dpred).all() and torch.isfinite(spec).all()
    assert s_err <= s_bar
    assert torch.equal(torch.sign(spec).double(), torch.sign(ref['spec64']))
    assert v_err <= v_bar
    assert g_err <= g_bar


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_two_sided_against_one_sided(K, case):
    """one spectrum for both modes; each value is the closed form on it: every term c (|Re| + |Im|) is one float32 rounding (2^-24) summed
    in double, the result rounded once more -- 2^-23 relative, asserted at twice that"""
    two, one = _device_run(K, (case, False)), _device_run(K, (case, True))
    assert torch.equal(two['spec'], one['spec'])
    w32 = float(np.float32(case[2]))
    for d, onesided in ((two, False), (one, True)):
        want = R.loss_from_spec(d['spec'].cpu(), case[0][3], w32, onesided)
        assert abs(float(d['loss'].item()) - want) <= 2 * R.ULP32 * want, (onesided, d['loss'].item(), want)


def test_zero_difference_is_exactly_zero(K):
    pred = torch.rand(2, 3, 48, 40, device='cuda')
    for onesided in R.MODES:
        loss, dpred, spec = K.freq_loss(pred, pred.clone(), 0.7, onesided, want_spectrum=True)
        assert loss.item() == 0.0 and (dpred == 0).all() and (spec == 0).all()


@pytest.mark.parametrize('run', [R.RUNS[0], R.RUNS[5], R.RUNS[12], R.RUNS[15], R.RUNS[17]], ids=R.run_id)
def test_accumulate_is_one_float32_add(K, run):
    d = _device_run(K, run)
    _, d_l1 = K.pixel_loss(K.LOSS_L1, d['pred'], d['gt'], 1.0, 0.0)
    acc = d_l1.clone()
    loss, out, spec = K.freq_loss(d['pred'], d['gt'], run[0][2], run[1], dpred=acc, want_spectrum=True)
    assert out.data_ptr() == acc.data_ptr()
    assert torch.equal(acc, d_l1 + d['dpred'])
    assert torch.equal(loss, d['loss']) and torch.equal(spec, d['spec'])


@pytest.mark.parametrize('run', [R.RUNS[6], R.RUNS[13], R.RUNS[14]], ids=R.run_id)
def test_power_of_two_scales_are_exact(K, run):
    from textualdegremoval_amd.optim import StepGuard
    d = _device_run(K, run)
    _, scaled = K.freq_loss(d['pred'], d['gt'], run[0][2], run[1], grad_scale=1024.0)
    assert torch.equal(scaled, d['dpred'] * 1024.0)
    guard = StepGuard(d['pred'].device)
    guard.write(scale=512.0, max_scale=512.0)
    _, guarded = K.freq_loss(d['pred'], d['gt'], run[0][2], run[1], guard=guard)
    assert torch.equal(guarded, d['dpred'] * 512.0)
    _, both = K.freq_loss(d['pred'], d['gt'], run[0][2], run[1], grad_scale=1024.0, guard=guard)
    assert torch.equal(both, d['dpred'] * (512.0 * 1024.0))


def _row_spectrum_in_ws(K, shape):
    """the half-spectrum region of the 'freq_loss' workspace (the last P H (W/2+1) complex of tdr_freq_loss_ws_bytes) as [P,H,W/2+1,2]"""
    from textualdegremoval_amd import _lib
    N, C, H, W = shape
    n = N * C * H * (W // 2 + 1) * 2
    total = _lib.load().tdr_freq_loss_ws_bytes(N, C, H, W) // 4
    ws = K.workspace(total, torch.device('cuda', torch.cuda.current_device()), 'freq_loss')
    return ws[total - n:total].clone().view(N * C, H, W // 2 + 1, 2)


@pytest.mark.parametrize('run', [R.RUNS[2], R.RUNS[9], R.RUNS[16], R.RUNS[19]], ids=R.run_id)
def test_value_only_writes_nothing_back_and_determinism(K, run):
    """dpred == NULL: the same loss bits, and the column pass stops after the partial sums -- the workspace still holds what the ROW pass
    wrote, the transform of d along W alone (held to the float64 rfft by the rule of this file: 8 x the float32 rfft's error, floor 4
    ulp), where a call with the gradient leaves the inverse column transform of the signs there, which is nowhere near it"""
    d = _device_run(K, run)
    case, onesided = run
    loss, none = K.freq_loss(d['pred'], d['gt'], case[2], onesided, want_grad=False)
    assert none is None and torch.equal(loss, d['loss'])
    after_value = _row_spectrum_in_ws(K, case[0]).cpu()
    d32 = R.reference(case, onesided)['d32']
    rows64 = torch.view_as_real(torch.fft.rfft(d32.double(), dim=-1)).reshape(after_value.shape)
    rows32 = torch.view_as_real(torch.fft.rfft(d32, dim=-1)).reshape(after_value.shape)
    err, bar = R.maxabs(after_value, rows64), R.bar(R.maxabs(rows32, rows64), rows64)
    print(f'{R.run_id(run)}: workspace after a value-only call against rfft along W: err {err:.3e} bar {bar:.3e}')
    assert err <= bar
    loss2, dpred2, spec2 = K.freq_loss(d['pred'], d['gt'], case[2], onesided, want_spectrum=True)
    assert torch.equal(loss2, d['loss']) and torch.equal(dpred2, d['dpred']) and torch.equal(spec2, d['spec'])
    after_grad = _row_spectrum_in_ws(K, case[0]).cpu()
    assert R.maxabs(after_grad, rows64) > 100 * bar           # the check above can tell the two apart
    again, _ = K.freq_loss(d['pred'], d['gt'], case[2], onesided, want_grad=False)
    assert torch.equal(again, d['loss'])
    assert torch.equal(_row_spectrum_in_ws(K, case[0]).cpu(), after_value)


def test_bad_arguments_launch_nothing(K):
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    n = 3 * 2048 * 8
    pred, gt = torch.rand(n, device='cuda'), torch.rand(n, device='cuda')
    sentinel, spec = torch.full((n,), -7.5, device='cuda'), torch.full((2 * n,), -7.5, device='cuda')
    loss = torch.full((1,), -7.5, device='cuda')
    ws = K.workspace(1 << 16, pred.device, 'freq_loss')
    ws.fill_(-7.5)
    st = torch.cuda.current_stream().cuda_stream

    def call(N, C, H, W, loss_ptr=loss.data_ptr(), pred_ptr=pred.data_ptr(), ws_ptr=ws.data_ptr()):
        return lib.tdr_freq_loss(pred_ptr, gt.data_ptr(), N, C, H, W, 0, 1.0, 1.0, None, 0, loss_ptr, sentinel.data_ptr(),
                                 spec.data_ptr(), ws_ptr, st)
    for H, W in ((6, 8), (7, 8), (2048, 8), (36, 8), (8, 6), (8, 2048), (0, 8), (8, 2)):
        assert lib.tdr_freq_loss_ws_bytes(1, 3, H, W) == 0, (H, W)
        assert call(1, 3, H, W) != 0, (H, W)
    for N, C in ((0, 3), (1, 0), (-1, 3), (65536, 1), (256, 256)):
        assert lib.tdr_freq_loss_ws_bytes(N, C, 8, 8) == 0, (N, C)
        assert call(N, C, 8, 8) != 0, (N, C)
    assert call(1, 3, 8, 8, loss_ptr=None) != 0
    assert call(1, 3, 8, 8, pred_ptr=None) != 0
    rc = call(1, 3, 8, 8, ws_ptr=None)
    assert rc != 0
    with pytest.raises(_lib.TdrError):
        _lib.check(rc, 'tdr_freq_loss')
    torch.cuda.synchronize()
    assert (sentinel == -7.5).all() and (spec == -7.5).all() and loss.item() == -7.5 and (ws == -7.5).all()


def test_python_errors(K):
    pred, gt = torch.rand(1, 3, 16, 16, device='cuda'), torch.rand(1, 3, 16, 16, device='cuda')
    with pytest.raises(ValueError):
        K.freq_loss(pred.double(), gt.double())
    with pytest.raises(ValueError):
        K.freq_loss(pred, gt.cpu())
    with pytest.raises(ValueError):
        K.freq_loss(pred.cpu(), gt)
    with pytest.raises(ValueError, match='1024'):
        K.freq_loss(torch.rand(1, 3, 36, 8, device='cuda'), torch.rand(1, 3, 36, 8, device='cuda'))
    with pytest.raises(ValueError):
        K.freq_loss(pred, gt[:, :, :8])


def test_autograd_through_the_module(K):
    from textualdegremoval_amd.losses import FFTLoss
    run = R.RUNS[15]
    d = _device_run(K, run)
    pred = d['pred'].clone().requires_grad_(True)
    gt = d['gt'].clone().requires_grad_(True)
    loss = FFTLoss(0.3, onesided=run[1])(pred, gt)
    loss.backward()
    want, dpred = K.freq_loss(d['pred'], d['gt'], 0.3, run[1])
    assert torch.equal(loss.detach().reshape(1), want)
    assert torch.equal(pred.grad, dpred) and gt.grad is None
    with pytest.raises(ValueError):
        FFTLoss()(torch.rand(1, 3, 100, 100, device='cuda'), torch.rand(1, 3, 100, 100, device='cuda'))
    with pytest.raises(ValueError):
        FFTLoss()(d['pred'].double(), d['gt'].double())
    with pytest.raises(ValueError):
        FFTLoss()(d['pred'], d['gt'].cpu())


def test_sfnet_recipe_over_three_scales(K):
    """sum over scales of L1 + FFTLoss(0.1): .backward() leaves each tensor the bits of the two kernels' dpred added"""
    from textualdegremoval_amd.losses import FFTLoss, L1Loss
    gen = torch.Generator().manual_seed(5)
    l1, freq = L1Loss(), FFTLoss(0.1)
    preds, gts, total = [], [], 0
    for s in (32, 16, 8):
        p = torch.rand(2, 3, s, s, generator=gen).cuda().requires_grad_(True)
        g = torch.rand(2, 3, s, s, generator=gen).cuda()
        preds.append(p)
        gts.append(g)
        total = total + l1(p, g) + freq(p, g)
    total.backward()
    want = 0.0
    for p, g in zip(preds, gts):
        la, da = K.pixel_loss(K.LOSS_L1, p.detach(), g, 1.0, 0.0)
        lb, db = K.freq_loss(p.detach(), g, 0.1)
        assert torch.equal(p.grad, da + db)
        want = want + la[0] + lb[0]
    assert torch.equal(total.detach(), want)
