"""The inference path of the Restormer family (RestormerRefFusion / Restormer, PromptIRRefFusion / PromptIR, DRSformerRefFusion /
DRSformer / DRSformer200L_SPA_RefFusion): `with torch.no_grad(): net(lq, ref)` runs the engine's net_fwd with keep=False -- the shared
walk of restormer_engine, nothing saved, `project_out` folded into the per-image attention weights (kernels.attn_fold_proj).
(1) the fold kernel against float64; (2) with restormer_engine.INFER_FOLD = False the no-grad forward is the grad-enabled forward bit
for bit; (3) with the fold it holds the 1e-4 parity bar of the whole-network golden tests; (4) nothing is kept and the route is taken;
(5) peak memory; (6) not slower; (7) validation between captured optimiser steps leaves the training run untouched."""
import functools
import gc
import os
import statistics

import numpy as np
import pytest
import torch

from oracle import drsformer_ref_oracle as DO
from oracle import nafnet_ref_oracle as NO
from oracle import promptir_ref_oracle as PO
from oracle import restormer_ref_oracle as RO

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MODES = ['bx3', 'f32', 'hx2']


def maxdiff(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


@pytest.fixture
def fold():
    """sets restormer_engine.INFER_FOLD for the duration of a test"""
    from textualdegremoval_amd import restormer_engine as R
    prev = R.INFER_FOLD

    def set_(on):
        R.INFER_FOLD = on
    yield set_
    R.INFER_FOLD = prev


# ------------------------------------------------------------------ (1) the fold kernel alone
def _poison(shape):
    """leaves NaNs in the block the allocator hands out next for `shape`: the kernel must write every element itself"""
    junk = torch.full(shape, float('nan'), device='cuda')
    torch.cuda.synchronize()
    del junk


@pytest.mark.parametrize('C,heads,attn', [(16, 2, 'mdta'), (24, 3, 'mdta'), (48, 1, 'mdta'), (192, 2, 'mdta'), (96, 8, 'mdta'), (24, 3, 'tksa')])
def test_fold_kernel_vs_float64(C, heads, attn):
    """Wf[n][j][r] = sum_{i in head(j)} Wo[r][i] AT[n][j][i] against the float64 product of the same fp32 inputs.  One fmaf chain of c
    terms: |error| <= gamma_c sum |terms| < c 2^-23 (|Wo| A) (A >= 0 here: the branch weights of the TKSA case are positive).  Cp > C
    (16, 24, 48), c no multiple of 64 (8, 12, 48, 96), c > 64 (96), more than one 16-row chunk per head and more than one 64-column
    tile (192, 96), a last chunk that is not full (c = 8, 12).  AT comes from tdr_mdta_softmax, and once from tdr_tksa_softmax."""
    from textualdegremoval_amd import kernels as K
    N, c = 2, C // heads
    gen = torch.Generator().manual_seed(100 * C + heads)
    G = torch.randn(N, C, C, generator=gen).cuda()
    ss = (0.5 + torch.rand(N, 2 * C, generator=gen)).cuda()
    temp = (1 + 0.3 * torch.randn(heads, 1, 1, generator=gen)).cuda()
    if attn == 'mdta':
        _, AT = K.mdta_softmax(G, ss, temp, heads)
    else:
        _, AT = K.tksa_softmax(G, ss, temp, (0.1 + torch.rand(4, generator=gen)).cuda(), heads)
    Wo = torch.randn(C, C, 1, 1, generator=gen).cuda()
    Cp = AT.shape[-1]
    assert Cp == K.mdta_pad(C) and AT.min().item() >= 0
    _poison((N, Cp, Cp))
    Wf = K.attn_fold_proj(AT, Wo, heads)
    assert Wf.shape == AT.shape
    A64, W64 = AT[:, :C, :C].double(), Wo.view(C, C).double()
    want = A64 @ W64.t()                                    # [n][j][r] = sum_i AT[n][j][i] Wo[r][i] (AT is zero outside head(j))
    bound = c * 2.0 ** -23 * (A64.abs() @ W64.abs().t())
    err = (Wf[:, :C, :C].double() - want).abs()
    print(f'C={C} heads={heads} {attn}: max |Wf - Wf64| {err.max().item():.3e}, max error / bound {(err / bound.clamp_min(1e-300)).max().item():.3f}')
    assert bool((err <= bound).all()), (err - bound).max().item()
    assert not Wf[:, C:, :].any() and not Wf[:, :, C:].any()          # the padding is written, as zeros
    _poison((N, Cp, Cp))
    assert torch.equal(K.attn_fold_proj(AT, Wo, heads), Wf)
    # what the fold is for: one convolution on Wf is project_out(attn v)
    prev = K.MATH
    K.set_math('f32')
    try:
        v = torch.randn(N, C, 8, 12, generator=gen).cuda()
        o = K.conv_forward(v, AT, Cp, C, 1, wp_ns=Cp * Cp)
        wp, mp, *_ = K.pack_weights(Wo, K.PACK_FWD)
        assert maxdiff(K.conv_forward(v, Wf, Cp, C, 1, wp_ns=Cp * Cp), K.conv_forward(o, wp, mp, C, 1)) < 1e-4
    finally:
        K.set_math(prev)


# ------------------------------------------------------------------ the whole-network cases of the three families
def _kw_drs(cfg):
    return {k: cfg[k] for k in ('inp_channels', 'out_channels', 'dim', 'num_blocks', 'heads', 'ffn_expansion_factor', 'bias',
                                'LayerNorm_type', 'nf', 'ext_n_blocks', 'reffusion_n_blocks', 'lr_block_size',
                                'ref_down_block_size', 'dilations', 'psize')}


def _restormer(kw):
    cfg = RO.default_cfg(**kw)
    return dict(type='RestormerRefFusion', **cfg), lambda seed: RO.synth_params(cfg, seed=seed), 4321


def _promptir(kw):
    cfg = PO.default_cfg(**kw)
    return dict(type='PromptIRRefFusion', **cfg), lambda seed: PO.synth_params(cfg, seed=seed), 8765


def _drsformer(kw):
    cfg = DO.default_cfg(**kw)
    return dict(type='DRSformer200L_SPA_RefFusion', **_kw_drs(cfg)), lambda seed: DO.synth_params(cfg, seed=seed), 8765


def _drsformer_mefc(kw):
    cfg = DO.default_cfg(**kw)
    return dict(type='DRSformerRefFusion', **_kw_drs(cfg)), lambda seed: DO.full_synth_params(dict(cfg, mefc=True), seed=seed), 8765


# (golden, family, constructor kwargs of the golden): the networks, weights and inputs of test_whole_net_vs_reference_golden /
# test_full_class_vs_reference_golden of test_hip_restormer.py, test_hip_promptir.py, test_hip_drsformer.py
GUIDED = [('restormer_d8_128', _restormer, dict()),
          ('restormer_d8_128_biasfree_b2', _restormer, dict(LayerNorm_type='BiasFree', num_blocks=[1, 2, 1, 1])),
          ('restormer_d8_64_wrap_bias', _restormer, dict(bias=True)),
          ('restormer_d16_120x100_pad', _restormer, dict(dim=16, nf=16)),
          ('promptir_d48_64', _promptir, dict()),
          ('promptir_d48_100x72_pad', _promptir, dict(bias=True)),
          ('drsformer_d8_64', _drsformer, dict()),
          ('drsformer_d16_100x72_pad', _drsformer, dict(dim=16, nf=16, bias=True)),
          ('drsformer_full_d8_64', _drsformer_mefc, dict())]
UNGUIDED = ['Restormer', 'PromptIR', 'DRSformer']
CASES = [g[0] for g in GUIDED] + UNGUIDED


def _build(case):
    """-> (net on the GPU, images, the reference's output or None)"""
    net, images, want = _make(case)
    return net.cuda(), tuple(t.cuda() for t in images), want


def _make(case):
    from textualdegremoval_amd.models.archs import define_network
    if case in UNGUIDED:
        x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(64))
        if case == 'Restormer':
            net = define_network(dict(type='Restormer', dim=8, num_blocks=[1, 2, 1, 1], num_refinement_blocks=1, heads=[1, 2, 2, 4], bias=True))
            P = RO.synth_params(RO.default_cfg(dim=8, nf=8, num_blocks=[1, 2, 1, 1], num_refinement_blocks=1, heads=[1, 2, 2, 4], bias=True), seed=2)
        elif case == 'PromptIR':
            cfg = PO.default_cfg(num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1])
            net = define_network(dict(type='PromptIR', dim=48, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, heads=cfg['heads'],
                                      ffn_expansion_factor=cfg['ffn_expansion_factor'], bias=cfg['bias'], LayerNorm_type=cfg['LayerNorm_type'],
                                      decoder=True))
            P = PO.synth_params(cfg, seed=2)
        else:
            cfg = DO.default_cfg(dim=16, nf=16, num_blocks=[1, 1, 1, 1], heads=[1, 2, 2, 4], ext_n_blocks=[1, 1, 1, 1], reffusion_n_blocks=[1, 1, 1, 1])
            net = define_network(dict(type='DRSformer', dim=16, num_blocks=[1, 1, 1, 1], heads=[1, 2, 2, 4],
                                      ffn_expansion_factor=cfg['ffn_expansion_factor'], bias=cfg['bias'], LayerNorm_type=cfg['LayerNorm_type']))
            P = DO.full_synth_params(dict(cfg, mefc=True), seed=2)
        net.load_state_dict({k: P[k] for k in net.state_dict()}, strict=True)
        return net, (x,), None
    name, family, kw = next(g for g in GUIDED if g[0] == case)
    g = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    seed = int(g['seed'])
    opt, params, seed0 = family(kw)
    net = define_network(opt)
    net.load_state_dict(params(seed), strict=True)
    lq, _, ref = NO.synth_pair(int(g['cfg_B']), int(g['cfg_H']), int(g['cfg_W']), seed=seed0 + seed)
    return net, (lq, ref), torch.from_numpy(g['out'])


@functools.lru_cache(maxsize=None)
def _outputs(case, mode):
    """one network per (case, arithmetic): (grad-enabled output, no-grad output without the fold, no-grad output with it, the reference's
    output or None) on the host -- computed once, read by the tests below.  The network itself is gone when this returns: the cache
    holds four small host tensors per entry.
    profiles/probe_restormer_infer.py imports CASES, MODES, maxdiff and this function from this module to record the same figures per
    case in its JSON: keep these four names when this file is reorganised."""
    from textualdegremoval_amd import kernels as K, restormer_engine as R
    prev_math, prev_fold = K.MATH, R.INFER_FOLD
    K.set_math(mode)
    try:
        net, images, want = _build(case)
        out_train = net(*images)
        assert out_train.grad_fn is not None
        outs = []
        for on in (False, True):
            R.INFER_FOLD = on
            with torch.no_grad():
                outs.append(net(*images))
            assert outs[-1].grad_fn is None and not outs[-1].requires_grad
        return out_train.detach().cpu(), outs[0].cpu(), outs[1].cpu(), want
    finally:
        K.set_math(prev_math)
        R.INFER_FOLD = prev_fold


# ------------------------------------------------------------------ (2) without the fold: the bits of the training forward
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES)
def test_no_grad_forward_without_fold_is_bit_identical(case, mode):
    out_train, out_nofold, _, _ = _outputs(case, mode)
    assert torch.equal(out_nofold, out_train), maxdiff(out_nofold, out_train)


# ------------------------------------------------------------------ (3) with the fold: the parity bar of the golden tests
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('case', CASES)
def test_no_grad_forward_with_fold_holds_the_parity_bar(case, mode):
    """max |out_no_grad - reference output| < 1e-4, the bar of test_whole_net_vs_reference_golden, and the same bar against the
    grad-enabled forward (the fold reassociates one c-term product per block; measured figures in DESIGN 5m)"""
    out_train, _, out_fold, want = _outputs(case, mode)
    d_train = maxdiff(out_fold, out_train)
    print(f'{case} {mode}: max |no-grad (fold) - grad-enabled| {d_train:.3e}' + ('' if want is None else f', - reference {maxdiff(out_fold, want):.3e}'
          f' (grad-enabled - reference {maxdiff(out_train, want):.3e})'))
    assert d_train < 1e-4
    if want is not None:
        assert maxdiff(out_fold, want) < 1e-4


# ------------------------------------------------------------------ (4) nothing kept, the route taken
def _spy(monkeypatch, engine):
    """records the `keep` every call of engine.net_fwd was made with and whether it returned something saved"""
    orig, seen = engine.net_fwd, []

    def wrapped(*a, **k):
        out, saved = orig(*a, **k)
        seen.append((k.get('keep', True), saved is None))
        return out, saved
    monkeypatch.setattr(engine, 'net_fwd', wrapped)
    return seen


@pytest.mark.parametrize('case', ['restormer_d8_64_wrap_bias', 'promptir_d48_64', 'drsformer_d8_64', 'drsformer_full_d8_64',
                                  'Restormer', 'PromptIR', 'DRSformer'])
def test_nothing_kept_and_route_taken(monkeypatch, case):
    from textualdegremoval_amd import drsformer_engine as DE, promptir_engine as PE, restormer_engine as R
    engine = R if 'estormer' in case else PE if 'rompt' in case else DE
    net, images, _ = _build(case)
    seen = _spy(monkeypatch, engine)
    out_train = net(*images)                               # grad mode, parameters that require grad: the autograd node, as before
    assert out_train.grad_fn is not None and seen == [(True, False)]
    with torch.no_grad():
        out = net(*images)
    assert seen[-1] == (False, True) and out.grad_fn is None and not out.requires_grad
    net.eval()                                             # .eval() alone selects nothing
    assert net(*images).grad_fn is not None and seen[-1] == (True, False)
    for p in net.parameters():                             # grad mode on, nothing that could ask for a gradient: the no-gradient route
        p.requires_grad_(False)
    out2 = net(*images)
    assert seen[-1] == (False, True) and out2.grad_fn is None and torch.equal(out2, out)
    out3 = net(images[0].clone().requires_grad_(True), *images[1:])      # (an input that requires grad: autograd again)
    assert seen[-1] == (True, False) and out3.requires_grad


# ------------------------------------------------------------------ (5), (6): the configs[2] network on one 256 x 256 image
CFG3 = dict(dim=48, nf=48, num_blocks=[4, 6, 6, 8], num_refinement_blocks=4, heads=[1, 2, 4, 8], ext_n_blocks=[4, 4, 4, 4],
            reffusion_n_blocks=[2, 2, 2, 2])


@functools.lru_cache(maxsize=None)
def _cfg3():
    from textualdegremoval_amd.models.archs import define_network
    cfg = RO.default_cfg(**CFG3)
    net = define_network(dict(type='RestormerRefFusion', **cfg))
    net.load_state_dict(RO.synth_params(cfg, seed=7), strict=True)
    lq, _, ref = NO.synth_pair(1, 256, 256, seed=77)
    return net.cuda(), lq.cuda(), ref.cuda()


@pytest.fixture
def bx3():
    from textualdegremoval_amd import kernels as K
    prev = K.MATH
    K.set_math('bx3')
    yield
    K.set_math(prev)


def _peak_delta(fn):
    """torch.cuda.max_memory_allocated() above what was allocated before fn() ran, fn's result still alive at the end"""
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def test_peak_memory_at_most_a_quarter(bx3):
    """Restormer-ref dim 48, blocks [4, 6, 6, 8], 4 refinement blocks, fusion [2, 2, 2, 2], 1 x 3 x 256 x 256.  The training forward keeps
    about 19 C-planes per TransformerBlock (twice that in the 2C-wide fusion blocks): about 500 level-0 C-planes by the end; the
    no-grad forward holds about 20 (x, y, t2, g of the 2C-wide first fusion block) plus the warped features and skips: a ratio near
    1 / 20 by count.  The bar -- the NAFNet family's -- leaves room for weight packs and workspaces, which appear on both sides: 1 / 4.
    The no-grad forward is measured before the grad-enabled one and once more after it."""
    net, lq, ref = _cfg3()

    def infer():
        with torch.no_grad():
            return net(lq, ref)
    first = _peak_delta(infer)
    train = _peak_delta(lambda: net(lq, ref))
    again = _peak_delta(infer)
    print(f'peak memory above the resident state: no-grad forward {again / 2**20:.0f} MiB (first call {first / 2**20:.0f} MiB), '
          f'grad-enabled forward {train / 2**20:.0f} MiB, ratio {again / train:.4f} (first call {first / train:.4f})')
    assert again <= train / 4 and first <= train / 4, (first, again, train)


def test_no_grad_forward_is_not_slower(bx3):
    """same process, same shape, alternating runs, medians of device time (two events around a run of three forwards): the grad-enabled
    forward is the parent's code path, unchanged -- the forward that launches, writes and allocates less must not take longer"""
    net, lq, ref = _cfg3()
    REP = 3

    def infer():
        with torch.no_grad():
            for _ in range(REP):
                net(lq, ref)

    def train():
        for _ in range(REP):
            net(lq, ref)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / REP
    for fn in (train, infer, train, infer):                # warm-up: code objects, workspaces, allocator
        timed(fn)
    t_train, t_infer = [], []
    for _ in range(11):
        t_train.append(timed(train))
        t_infer.append(timed(infer))
    mt, mi = statistics.median(t_train), statistics.median(t_infer)
    print(f'Restormer-ref forward at 1x3x256x256: grad-enabled median {mt:.2f} ms (min {min(t_train):.2f}), no-grad median {mi:.2f} ms '
          f'(min {min(t_infer):.2f})')
    assert mi <= mt, (t_infer, t_train)


# ------------------------------------------------------------------ (7) validation between captured optimiser steps
def _trainer(seed):
    from textualdegremoval_amd.models import create_model
    cfg = RO.default_cfg()
    model = create_model({
        'model_type': 'RefGuidedImageCleanModel', 'num_gpu': 1, 'dist': False, 'is_train': True,
        'network_g': dict(type='RestormerRefFusion', **cfg), 'path': {},
        'train': {'optim_g': {'type': 'AdamW', 'lr': 2e-4, 'ref_lr': 1e-4, 'weight_decay': 1e-4, 'betas': [0.9, 0.999]},
                  'scheduler': {'type': 'CosineAnnealingRestartCyclicLR', 'periods': [30, 70], 'restart_weights': [1, 1],
                                'eta_mins': [3e-4, 1e-6]},
                  'pixel_opt': {'type': 'L1Loss', 'loss_weight': 1, 'reduction': 'mean'},
                  'use_grad_clip': True, 'total_iter': 100, 'warmup_iter': -1},
        'logger': {'check_freq': 10 ** 9}, 'val': {}, 'scale': 1})
    model.net_g.load_state_dict(RO.synth_params(cfg, seed=seed), strict=True)
    return model


def test_validation_between_captured_steps(monkeypatch, fold):
    """RefGuidedImageCleanModel on RestormerRefFusion with the hipGraph step (eager, eager, capture + replay, replay, replay): nonpad_test
    after steps 3 and 5 reads the weights the optimiser has just written -- without the fold its output is the grad-enabled forward of the
    current parameters bit for bit, with it within 1e-4 -- and the loss trajectory is that of a run that never validated.
    (kernels.DETERMINISTIC: the one order-dependent reduction of the step accumulates in fixed point.)"""
    from textualdegremoval_amd import kernels as K
    monkeypatch.setenv('TDR_GRAPH', '1')
    monkeypatch.setattr(K, 'DETERMINISTIC', True)
    lq, gt, ref = NO.synth_pair(1, 128, 128, seed=4321 + 3)
    vlq, _, vref = NO.synth_pair(1, 200, 136, seed=99)                        # a validation image of another size than the step's

    def run(validate_after):
        model = _trainer(3)
        losses, vals = [], []
        for it in range(1, 6):
            model.update_learning_rate(it, warmup_iter=-1)
            model.feed_train_data({'lq': lq, 'gt': gt, 'ref': ref})
            model.optimize_parameters(it)
            losses.append(model.get_current_log()['l_pix'])
            if it in validate_after:
                for a, b in ((lq, ref), (vlq, vref)):
                    model.feed_data({'lq': a, 'ref': b})
                    want = None
                    for on in (False, True):
                        fold(on)
                        model.nonpad_test()
                        assert not model.output.requires_grad and model.net_g.training
                        if want is None:
                            want = model.net_g(model.lq, model.ref)          # grad-enabled forward of the current parameters
                            assert want.grad_fn is not None
                            want = want.detach()
                        if on:
                            assert maxdiff(model.output, want) < 1e-4, (it, maxdiff(model.output, want))
                        else:
                            assert torch.equal(model.output, want), (it, maxdiff(model.output, want))
                    vals.append(model.output.clone())
        assert model._gstate['segs'] is not None                         # the step was captured and replayed
        return losses, vals
    plain, _ = run(())
    with_val, vals = run((3, 5))
    assert with_val == plain, (with_val, plain)
    assert len(vals) == 4 and not torch.equal(vals[0], vals[2])          # two more optimiser steps lie between the validations
