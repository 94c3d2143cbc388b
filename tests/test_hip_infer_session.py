"""inference.InferenceSession on the GPU: (1) every call -- eager, capture + replay, replay -- gives the bits of `with torch.no_grad():
net(...)`, (2) a replay runs no Python forward and packs no parameter, and the plan stops growing, (3) refresh() / moved parameters,
(4) several shapes through the LRU and release(), (5) the byte kernels of csrc/tdr_imgio.hip against numpy restatements of the reference's
imfrombytes / img2tensor / tensor2img, (6) the step model with `val: {session: true}` keeps its trajectory and reads current weights."""
import gc
import os

import numpy as np
import pytest
import torch

from oracle import nafnet_ref_oracle as O

import test_hip_dynfusion_inference as TD
import test_hip_inference as TI
import test_hip_restormer_inference as TR
import test_hip_tlsc_fused as TL

pytestmark = pytest.mark.gpu
GOLDEN = TI.GOLDEN
W8 = TI.W8
MODES = ['bx3', 'f32', 'hx2']


@pytest.fixture
def set_math():
    from textualdegremoval_amd import kernels as K
    prev = K.MATH
    yield K.set_math
    K.set_math(prev)


# ------------------------------------------------------------------ the networks: name -> (net, images, (engine module, forward name))
def _guided(name, ref_hw):
    from textualdegremoval_amd import engine as E
    g = np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False)
    seed = int(g['seed'])
    lq, _, ref = O.synth_pair(int(g['cfg_B']), int(g['cfg_H']), int(g['cfg_W']), seed=1234 + seed, ref_hw=ref_hw)
    return TI._guided_net(W8, seed), (lq.cuda(), ref.cuda()), (E, 'net_fwd')


def _nafnet_w32():
    from textualdegremoval_amd import engine as E
    from textualdegremoval_amd.models.archs import define_network
    net = define_network(dict(type='NAFNet', img_channel=3, width=32, middle_blk_num=1, enc_blk_nums=[1, 1, 1], dec_blk_nums=[1, 1, 1]))
    torch.manual_seed(5)
    for k, p in net.named_parameters():
        if k.endswith(('beta', 'gamma')):
            torch.nn.init.normal_(p, std=0.3)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(3))
    return net.cuda(), (x.cuda(),), (E, 'unet_fwd')


def _local():
    from textualdegremoval_amd import engine as E
    g, net = TL._golden_net()
    net.load_state_dict({str(k): torch.from_numpy(g['p_' + str(k)]) for k in g['names']}, strict=True)
    return net.cuda(), (torch.from_numpy(g['x']).cuda(),), (E, 'unet_fwd')


def _restormer_walk(case):
    def make():
        from textualdegremoval_amd import drsformer_engine as DE, promptir_engine as PE, restormer_engine as R
        net, images, _ = TR._build(case)
        eng = PE if 'romptir' in case.lower() or case == 'PromptIR' else DE if 'drsformer' in case.lower() else R
        return net, images, (eng, 'net_fwd')
    return make


def _dynfusion():
    from textualdegremoval_amd import dynfusion_engine as D
    x, kv, _, _ = TD._draw_inputs(TD.CASES['a'][0], *TD.CASES['a'][1])
    return TD._golden_net(), (torch.from_numpy(x).cuda(), torch.from_numpy(kv).cuda()), (D, 'dyn_unet_fwd')


NETS = {'NAFNetRefFusion-256-b2': lambda: _guided('net_w8_256_b2_clear', None),
        'NAFNetRefFusion-120x100-pad': lambda: _guided('net_w8_120x100_pad', None),
        'NAFNetRefFusion-256-ref384': lambda: _guided('net_w8_256_ref384', (384, 384)),
        'NAFNet-w32': _nafnet_w32, 'NAFNetLocal': _local, 'RestormerRefFusion': _restormer_walk('restormer_d8_64_wrap_bias'),
        'NAFNetDynamicFusion': _dynfusion}
# the other classes on the shared Restormer walk, through the same route (default arithmetic)
WALK = {c: _restormer_walk(c) for c in ('Restormer', 'PromptIR', 'DRSformer', 'promptir_d48_64', 'drsformer_d8_64', 'drsformer_full_d8_64')}


def _other_content(images, seed):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for t in images:
        r = torch.randn(t.shape, generator=gen) if t.dim() == 3 else torch.rand(t.shape, generator=gen)      # (k_v is [N, 10, 1024])
        out.append(r.cuda())
    return tuple(out)


def _eager(net, images):
    with torch.no_grad():
        return net(*images)


class _Spies:
    """Python calls of the engine's whole-network forward; pack launches, split into those of admitted weights (parameters) and others"""

    def __init__(self, monkeypatch, sess, engine):
        from textualdegremoval_amd import kernels as K
        self.forward, self.admitted, self.derived, self.multi = 0, 0, 0, 0
        mod, name = engine
        orig_fwd, orig_pack = getattr(mod, name), K._pack_into
        lib = K._lib.load()
        orig_multi = lib.tdr_pack_weights_multi

        def fwd(*a, **k):
            self.forward += 1
            return orig_fwd(*a, **k)

        def pack(w, mode, pw):
            if w.data_ptr() in sess.plan.admit:
                self.admitted += 1
            else:
                self.derived += 1
            return orig_pack(w, mode, pw)

        def multi(*a):
            self.multi += 1
            return orig_multi(*a)
        monkeypatch.setattr(mod, name, fwd)
        monkeypatch.setattr(K, '_pack_into', pack)
        monkeypatch.setattr(lib, 'tdr_pack_weights_multi', multi)

    def counts(self):
        return self.forward, self.admitted, self.multi


def _three_calls(monkeypatch, make):
    from textualdegremoval_amd.inference import InferenceSession
    net, images, engine = make()
    other = _other_content(images, 17)
    want, want_other = _eager(net, images), _eager(net, other)
    assert not torch.equal(want, want_other)
    sess = InferenceSession(net, max_graphs=4)
    spy = _Spies(monkeypatch, sess, engine)
    out1 = sess(*images)                                                     # call 1: eager under the session's plan
    n_entries = len(sess.plan.entries)
    assert spy.forward == 1 and spy.admitted == n_entries > 0 and sess.captures == 0
    assert torch.equal(out1, want), (out1 - want).abs().max().item()
    before = spy.counts()
    out2 = sess(*images)                                                     # call 2: capture (one Python forward) + replay
    assert sess.captures == 1 and sess.replays == 1 and spy.forward == before[0] + 1
    assert (spy.admitted, spy.multi) == before[1:], 'call 2 packed a parameter'
    assert torch.equal(out2, want), (out2 - want).abs().max().item()
    assert len(sess.plan.entries) == n_entries
    before = spy.counts()
    out3 = sess(*other)                                                      # call 3: replay on other content
    assert spy.counts() == before, 'call 3 ran Python forward code or packed a parameter'
    assert sess.captures == 1 and sess.replays == 2
    assert torch.equal(out3, want_other), (out3 - want_other).abs().max().item()
    assert torch.equal(out2, want)                                           # what the caller holds is not overwritten by a later replay
    for i in range(4, 11):
        out = sess(*(images if i % 2 else other))
    assert torch.equal(out, want_other) and len(sess.plan.entries) == n_entries and spy.counts() == before
    print(f'{type(net).__name__}: {n_entries} packed weights, {spy.derived} packs of derived weights in calls 1 - 2')
    sess.release()
    return spy


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('name', list(NETS))
def test_three_calls_bit_identical_and_a_replay_is_a_replay(monkeypatch, set_math, name, mode):
    set_math(mode)
    _three_calls(monkeypatch, NETS[name])


@pytest.mark.parametrize('name', list(WALK))
def test_other_classes_of_the_restormer_walk(monkeypatch, name):
    _three_calls(monkeypatch, WALK[name])


# ------------------------------------------------------------------ weights
def test_refresh_and_moved_parameters():
    from textualdegremoval_amd.inference import InferenceSession
    net = TI._guided_net(W8, 3)
    lq, _, ref = O.synth_pair(1, 128, 128, seed=1237)
    lq, ref = lq.cuda(), ref.cuda()
    sess = InferenceSession(net)
    for _ in range(3):
        out0 = sess(lq, ref)
    assert torch.equal(out0, _eager(net, (lq, ref))) and sess.captures == 1
    with torch.no_grad():
        for p in net.parameters():
            p.mul_(1.01)
    want = _eager(net, (lq, ref))
    assert not torch.equal(want, out0)
    assert not torch.equal(sess(lq, ref), want)                              # not refreshed: stale packs under current biases / norms (the documented contract)
    sess.refresh()
    assert torch.equal(sess(lq, ref), want) and sess.captures == 1 and sess.rebuilds == 1        # re-packed; the graph stayed
    ptrs = [p.data_ptr() for p in net.parameters()]
    net.load_state_dict({k: v * 0.98 for k, v in net.state_dict().items()}, strict=True)
    assert ptrs == [p.data_ptr() for p in net.parameters()]
    sess.refresh()
    want2 = _eager(net, (lq, ref))
    assert not torch.equal(want2, want) and torch.equal(sess(lq, ref), want2) and sess.captures == 1
    p = net.ending.weight                                                    # new storage: noticed at the next call without refresh()
    p.data = p.data.clone() * 1.05
    assert p.data_ptr() not in ptrs
    want3 = _eager(net, (lq, ref))
    assert not torch.equal(want3, want2)
    for _ in range(3):
        assert torch.equal(sess(lq, ref), want3)
    assert sess.rebuilds == 2 and sess.captures == 2
    sess.release()


# ------------------------------------------------------------------ shapes
def test_two_shapes_alternate_lru_recaptures_and_release_frees():
    from textualdegremoval_amd.inference import InferenceSession
    net, (a,), _ = _nafnet_w32()
    b = torch.rand(1, 3, 32, 96, generator=torch.Generator().manual_seed(4)).cuda()         # (the depthwise stencil wants W / 8 % 4 == 0)
    want = {id(a): _eager(net, (a,)), id(b): _eager(net, (b,))}
    gc.collect()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    sess = InferenceSession(net, max_graphs=2)
    for x in (a, b, a, b, a, b, a, b):
        assert torch.equal(sess(x), want[id(x)])
    assert sess.captures == 2 and sess.replays == 6 and len(sess.graphs) == 2
    one = InferenceSession(net, max_graphs=1)
    for x in (a, a, b, b, a, a, b):
        assert torch.equal(one(x), want[id(x)])
    assert one.captures == 4 and len(one.graphs) == 1                        # a, b, a again, b again: the evicted shape is captured anew
    zero = InferenceSession(net, max_graphs=0)
    for x in (a, a, b, a):
        assert torch.equal(zero(x), want[id(x)])
    assert zero.captures == 0 and len(zero.plan.entries) == len(sess.plan.entries)
    packs = sum(e[3].buf.numel() * 4 for e in sess.plan.entries.values())
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    for s in (sess, one, zero):
        s.release()
    del sess, one, zero, x
    gc.collect()
    torch.cuda.synchronize()
    left = torch.cuda.memory_allocated() - base
    print(f'three sessions held {held / 2**20:.1f} MiB ({packs / 2**20:.2f} MiB of packs each); {left} bytes left after release()')
    assert held > packs and left <= packs


# ------------------------------------------------------------------ byte kernels against numpy
def np_u8_to_planes(img, swap, Hp, Wp):
    """imfrombytes(float32=True) + img2tensor(bgr2rgb=swap) of utils/utils_image.py, per image of the batch, + the zero pad"""
    x = img.astype(np.float32) / 255.
    if img.shape[3] == 3 and swap:
        x = x[..., ::-1]                                                     # cv2.cvtColor(img, cv2.COLOR_BGR2RGB)
    x = x.transpose(0, 3, 1, 2)
    out = np.zeros(x.shape[:2] + (Hp, Wp), np.float32)
    out[:, :, :x.shape[2], :x.shape[3]] = x
    return out


def np_planes_to_u8(planes, swap, H, W):
    """tensor2img(rgb2bgr=swap, out_type=np.uint8, min_max=(0, 1)) of utils/utils_image.py on the top-left (H, W)"""
    t = torch.from_numpy(np.ascontiguousarray(planes[:, :, :H, :W])).float().clamp_(0, 1)
    t = (t - 0) / (1 - 0)
    img = t.numpy().transpose(0, 2, 3, 1)
    if img.shape[3] == 3 and swap:
        img = img[..., ::-1]                                                 # cv2.cvtColor(img_np, cv2.COLOR_RGB2BGR)
    return (img * 255.0).round().astype(np.uint8)


@pytest.mark.parametrize('swap', [False, True])
def test_u8_to_planes_bit_exact(swap):
    from textualdegremoval_amd import kernels as K
    rng = np.random.default_rng(1)
    ramp = np.arange(256, dtype=np.uint8)
    cases = [(ramp.reshape(1, 16, 16, 1), 16, 32), (np.repeat(ramp, 3).reshape(1, 16, 16, 3), 16, 16)]
    for shape in ((1, 5, 7, 3), (2, 16, 20, 1), (1, 8, 12, 6)):
        img = rng.integers(0, 256, size=shape, dtype=np.uint8)
        cases += [(img, 16, 32), (img, shape[1], shape[2]), (img, shape[1] + 1, shape[2] + 3)]       # padded; as is; a pitch off 16 bytes
    for img, Hp, Wp in cases:
        got = K.img_u8_to_planes(torch.from_numpy(img).cuda(), Hp, Wp, swap_rb=swap).cpu().numpy()
        want = np_u8_to_planes(img, swap, Hp, Wp)
        assert got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (img.shape, Hp, Wp)
    assert len(set(np_u8_to_planes(cases[0][0], swap, 16, 16).ravel().tolist())) == 256


@pytest.mark.parametrize('swap', [False, True])
def test_planes_to_u8_bit_exact(swap):
    from textualdegremoval_amd import kernels as K
    rng = np.random.default_rng(2)
    cases = []
    for N, H, W, C in ((1, 5, 7, 3), (2, 16, 20, 1), (1, 8, 12, 6)):
        planes = rng.uniform(-0.2, 1.2, size=(N, C, 16, 32)).astype(np.float32)
        cases += [(planes, H, W), (np.ascontiguousarray(planes[:, :, :H, :W]), H, W), (np.ascontiguousarray(planes[:, :, :H + 1, :W + 3]), H, W)]
    # every k / 255 and the float32 neighbours of every (k + 0.5) / 255: the ties of the rounding
    exact = (np.arange(256, dtype=np.float32) / np.float32(255.)).astype(np.float32)
    mid = ((np.arange(255, dtype=np.float64) + 0.5) / 255.).astype(np.float32)
    vals = np.concatenate([exact, mid, np.nextafter(mid, np.float32(-1)), np.nextafter(mid, np.float32(2)), np.zeros(3, np.float32)])
    assert vals.size == 1024 and vals.dtype == np.float32
    cases += [(vals.reshape(1, 1, 32, 32), 32, 32), (np.stack([vals, vals[::-1], np.roll(vals, 5)]).reshape(1, 3, 32, 32), 32, 32)]
    for planes, H, W in cases:
        assert np.isfinite(planes).all()
        got = K.planes_to_img_u8(torch.from_numpy(planes).cuda(), H, W, swap_rb=swap).cpu().numpy()
        want = np_planes_to_u8(planes, swap, H, W)
        assert got.shape == want.shape == (planes.shape[0], H, W, planes.shape[1]) and np.array_equal(got, want), (planes.shape, H, W)
    # and back: every byte survives the round trip
    ramp = torch.arange(256, dtype=torch.uint8).view(1, 16, 16, 1).cuda()
    assert torch.equal(K.planes_to_img_u8(K.img_u8_to_planes(ramp, 16, 32, swap_rb=swap), 16, 16, swap_rb=swap), ramp)


@pytest.mark.parametrize('bgr', [True, False])
def test_run_u8_is_the_two_kernels_around_the_session(bgr):
    from textualdegremoval_amd import kernels as K
    from textualdegremoval_amd.inference import InferenceSession
    net = TI._guided_net(W8, 3)
    rng = np.random.default_rng(3)
    sess = InferenceSession(net)
    for i in range(4):                                                       # eager, capture + replay, replay, replay; new bytes each time
        lq = torch.from_numpy(rng.integers(0, 256, size=(1, 120, 100, 3), dtype=np.uint8)).cuda()
        ref = torch.from_numpy(rng.integers(0, 256, size=(1, 120, 100, 3), dtype=np.uint8)).cuda()
        got = sess.run_u8(lq, ref, bgr=bgr)
        want = K.planes_to_img_u8(_eager(net, (K.img_u8_to_planes(lq, swap_rb=bgr), K.img_u8_to_planes(ref, swap_rb=bgr))), swap_rb=bgr)
        assert got.dtype == torch.uint8 and got.shape == lq.shape and torch.equal(got, want), i
        planes = sess(K.img_u8_to_planes(lq, swap_rb=bgr), K.img_u8_to_planes(ref, swap_rb=bgr))
        assert torch.equal(K.planes_to_img_u8(planes, swap_rb=bgr), got)
    assert sess.captures == 2 and len(sess.graphs) == 2                      # the byte pipeline and the plane forward: a graph each
    sess.release()


# ------------------------------------------------------------------ the step model
def test_step_model_with_val_session_keeps_the_trajectory(monkeypatch):
    """the five-step pattern of test_hip_inference.py (eager, eager, capture + replay, replay, replay; validation after steps 3 and 5) with
    `val: {session: true}` and without: the same losses, the same validation outputs bit for bit, and validation reads current weights"""
    from textualdegremoval_amd import kernels as K
    monkeypatch.setenv('TDR_GRAPH', '1')
    monkeypatch.setattr(K, 'DETERMINISTIC', True)
    lq, gt, ref = O.synth_pair(1, 128, 128, seed=1234 + 3)
    vlq, _, vref = O.synth_pair(1, 200, 136, seed=99, ref_hw=(300, 300))

    def run(session):
        model = TI._trainer(3)
        if session:
            model.opt['val'] = {'session': True}
        losses, vals = [], []

        def loader():
            for a, b in ((lq, ref), (vlq, vref)):
                yield {'lq': a, 'ref': b}
                vals.append(model.output.clone())
        for it in range(1, 6):
            model.update_learning_rate(it, warmup_iter=-1)
            model.feed_train_data({'lq': lq, 'gt': gt, 'ref': ref})
            model.optimize_parameters(it)
            losses.append(model.get_current_log()['l_pix'])
            if it in (3, 5):
                model.nondist_validation(loader(), it, None, False, True, True)
                assert model.net_g.training and not model.output.requires_grad
        assert model._gstate['segs'] is not None
        sessions = list(getattr(model, '_val_sessions', {}).values())
        assert len(sessions) == (1 if session else 0)
        if session:
            assert sessions[0].net is model.net_g and sessions[0].captures == 2 and sessions[0].replays == 2
            model.feed_data({'lq': lq, 'ref': ref})                          # a bare nonpad_test re-packs by itself
            model.nonpad_test()
            assert torch.equal(model.output, vals[2])
        return losses, vals
    plain, vals_plain = run(False)
    with_session, vals = run(True)
    assert with_session == plain, (with_session, plain)
    assert len(vals) == len(vals_plain) == 4 and all(torch.equal(a, b) for a, b in zip(vals, vals_plain))
    assert not torch.equal(vals[0], vals[2])
