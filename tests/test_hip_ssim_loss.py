"""tdr_ssim_loss on the GPU (csrc/tdr_ssim_loss.hip) through kernels.ssim_loss and losses.SSIMLoss: the forward pinned to the bits of
tdr_ssim3d, the gradient held to the float64 reference of tests/_ssim_loss_ref.py by the rule of tests/test_hip_masa_kernels.py --
max|dpred - dpred64| <= max(8 e32, 4 float32 ulp of max|dpred64|), e32 the error of the same reference run in float32; no bar is typed in.

Measured on an MI355X (profiles/ssim_loss/errors.txt holds the printed lines of every case): max|dpred - dpred64| is 3.3e-7 - 1.7e-6 of
the tensor maximum in all 26 cases, e32 5.4e-7 - 6.8e-5 of it; the value is 2e-9 - 1.1e-7 from the float64 loss."""
import pytest
import torch

import _ssim_loss_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    from textualdegremoval_amd import kernels
    return kernels


_dev = {}


def _device_case(K, case):
    """inputs on the device and ONE kernel run per case, shared read-only by the tests"""
    if case not in _dev:
        ref = R.reference(case)
        pred, gt = ref['pred'].cuda(), ref['gt'].cuda()
        loss, ssim, dpred = K.ssim_loss(pred, gt, R.WEIGHT, case[2])
        _dev[case] = dict(pred=pred, gt=gt, loss=loss, ssim=ssim, dpred=dpred)
    return _dev[case]


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_forward_is_ssim3d_bit_for_bit(K, case):
    d = _device_case(K, case)
    for n in range(case[0][0]):
        one = K.ssim3d(d['pred'][n].permute(1, 2, 0).contiguous(), d['gt'][n].permute(1, 2, 0).contiguous(), case[2])
        assert torch.equal(d['ssim'][n:n + 1], one), (n, d['ssim'][n].item(), one.item())
    assert d['loss'].cpu().numpy()[0] == R.host_loss(d['ssim'], R.WEIGHT)


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_value_against_float64(K, case):
    d, ref = _device_case(K, case), R.reference(case)
    err = abs(float(d['loss'].item()) - ref['loss64'])
    print(f'{R.case_id(case)}: |loss - loss64| {err:.2e} (bar {2e-4 * R.WEIGHT:.1e}; the float32 reference: {ref["v32"]:.2e})')
    assert err <= 2e-4 * R.WEIGHT


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_gradient_against_float64(K, case):
    d, ref = _device_case(K, case), R.reference(case)
    err, bar = R.maxabs(d['dpred'].cpu(), ref['dpred64']), R.bar(ref['e32'], ref['dpred64'])
    top = ref['dpred64'].abs().max().item()
    print(f'{R.case_id(case)}: max|dpred - dpred64| {err:.3e}  e32 {ref["e32"]:.3e}  bar {bar:.3e}  max|dpred64| {top:.3e}  '
          f'(kernel / max {err / top:.1e}, e32 / max {ref["e32"] / top:.1e})')
    assert torch.isfinite(d['dpred']).all()
    assert err <= bar


@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[3], R.CASES[9], R.CASES[14], R.CASES[-1]], ids=R.case_id)
def test_accumulate_is_one_float32_add(K, case):
    d = _device_case(K, case)
    _, d_l1 = K.pixel_loss(K.LOSS_L1, d['pred'], d['gt'], 1.0, 0.0)
    acc = d_l1.clone()
    loss, ssim, out = K.ssim_loss(d['pred'], d['gt'], R.WEIGHT, case[2], dpred=acc)
    assert out.data_ptr() == acc.data_ptr()
    assert torch.equal(acc, d_l1 + d['dpred'])
    assert torch.equal(loss, d['loss']) and torch.equal(ssim, d['ssim'])


@pytest.mark.parametrize('case', [R.CASES[3], R.CASES[9], R.CASES[20]], ids=R.case_id)
def test_power_of_two_scales_are_exact(K, case):
    from textualdegremoval_amd.optim import StepGuard
    d = _device_case(K, case)
    _, _, scaled = K.ssim_loss(d['pred'], d['gt'], R.WEIGHT, case[2], grad_scale=1024.0)
    assert torch.equal(scaled, d['dpred'] * 1024.0)
    guard = StepGuard(d['pred'].device)
    guard.write(scale=512.0, max_scale=512.0)
    _, _, guarded = K.ssim_loss(d['pred'], d['gt'], R.WEIGHT, case[2], guard=guard)
    assert torch.equal(guarded, d['dpred'] * 512.0)
    _, _, both = K.ssim_loss(d['pred'], d['gt'], R.WEIGHT, case[2], grad_scale=1024.0, guard=guard)
    assert torch.equal(both, d['dpred'] * (512.0 * 1024.0))


@pytest.mark.parametrize('case', [R.CASES[0], R.CASES[9], R.CASES[16]], ids=R.case_id)
def test_value_only_and_determinism(K, case):
    d = _device_case(K, case)
    loss, ssim, none = K.ssim_loss(d['pred'], d['gt'], R.WEIGHT, case[2], want_grad=False)
    assert none is None
    assert torch.equal(loss, d['loss']) and torch.equal(ssim, d['ssim'])
    loss2, ssim2, dpred2 = K.ssim_loss(d['pred'], d['gt'], R.WEIGHT, case[2])
    assert torch.equal(loss2, d['loss']) and torch.equal(ssim2, d['ssim']) and torch.equal(dpred2, d['dpred'])


def test_bad_arguments_launch_nothing(K):
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    pred, gt = torch.rand(1, 5, 8, 8, device='cuda'), torch.rand(1, 5, 8, 8, device='cuda')
    sentinel = torch.full_like(pred, -7.5)
    with pytest.raises(_lib.TdrError):
        K.ssim_loss(pred, gt, dpred=sentinel)
    torch.cuda.synchronize()
    assert (sentinel == -7.5).all()
    assert lib.tdr_ssim_loss_ws_bytes(1, 5, 8, 8) == 0 and lib.tdr_ssim_loss_ws_bytes(1, 3, 0, 8) == 0
    # H = 0 with real buffers behind every pointer
    loss, ssim = torch.full((1,), -7.5, device='cuda'), torch.full((1,), -7.5, device='cuda')
    ws = K.workspace(1 << 16, pred.device, 'ssim_loss')
    rc = lib.tdr_ssim_loss(pred.data_ptr(), gt.data_ptr(), 1, 3, 0, 8, 1.0, 1.0, 1.0, None, 0, loss.data_ptr(), ssim.data_ptr(),
                           sentinel.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    with pytest.raises(_lib.TdrError):
        _lib.check(rc, 'tdr_ssim_loss')
    rc = lib.tdr_ssim_loss(pred.data_ptr(), gt.data_ptr(), 1, 3, 8, 8, 1.0, 1.0, 1.0, None, 0, None, ssim.data_ptr(),
                           sentinel.data_ptr(), ws.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc != 0
    torch.cuda.synchronize()
    assert (sentinel == -7.5).all() and loss.item() == -7.5 and ssim.item() == -7.5
    with pytest.raises(ValueError):
        K.ssim_loss(pred.double(), gt.double())


def test_autograd_through_the_module(K):
    from textualdegremoval_amd.losses import SSIMLoss
    case = R.CASES[9]
    d = _device_case(K, case)
    pred = d['pred'].clone().requires_grad_(True)
    gt = d['gt'].clone().requires_grad_(True)
    loss = SSIMLoss(0.3)(pred, gt)
    loss.backward()
    l, _, dpred = K.ssim_loss(d['pred'], d['gt'], 0.3, 1.0)
    assert torch.equal(loss.detach().reshape(1), l)
    assert torch.equal(pred.grad, dpred) and gt.grad is None
    with pytest.raises(ValueError):
        SSIMLoss()(torch.rand(1, 5, 8, 8, device='cuda'), torch.rand(1, 5, 8, 8, device='cuda'))
    with pytest.raises(ValueError):
        SSIMLoss()(d['pred'].double(), d['gt'].double())
    with pytest.raises(ValueError):
        SSIMLoss()(d['pred'], d['gt'].cpu())
