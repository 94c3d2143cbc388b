"""Host-side bookkeeping of inference.InferenceSession (no GPU): the LRU of captured graphs, the key a graph is valid for, the admit-set of
kernels.PackPlan on fake pointers, the eager / capture / replay policy with the capture itself replaced by a recorder, and the two things
a session notices on its own (moved parameters, another arithmetic)."""
import pytest
import torch
import torch.nn as nn

from textualdegremoval_amd import inference as I
from textualdegremoval_amd import kernels as K


def test_lru_evicts_least_recently_used_first():
    lru = I.GraphLRU(2)
    assert lru.make_room() == [] and len(lru) == 0
    lru.put('a', 1)
    assert lru.make_room() == []
    lru.put('b', 2)
    assert lru.get('a') == 1 and lru.keys() == ['b', 'a']          # a touch moves an entry to the young end
    assert lru.make_room() == [2] and lru.keys() == ['a']          # room for ONE more: the oldest goes
    lru.put('c', 3)
    assert lru.get('b') is None and lru.get('zzz') is None
    assert lru.get('a') == 1 and lru.make_room() == [3]
    lru.put('d', 4)
    assert lru.keys() == ['a', 'd']
    one = I.GraphLRU(1)
    one.put('x', 'X')
    assert one.make_room() == ['X'] and len(one) == 0
    lru.clear()
    assert len(lru) == 0


def test_key_is_shapes_dtypes_math_and_entry_point():
    a, b = torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 12, 12)
    k = I.session_key([a, b], 'bx3')
    assert k == ((((1, 3, 8, 8), 'torch.float32'), ((1, 3, 12, 12), 'torch.float32')), 'bx3', None)
    assert I.session_key([a.clone() + 1, b.clone()], 'bx3') == k                       # content does not matter
    assert I.session_key([b, a], 'bx3') != k and I.session_key([a, b], 'hx2') != k
    assert I.session_key([a, None], 'bx3') == ((((1, 3, 8, 8), 'torch.float32'), None), 'bx3', None) != I.session_key([a], 'bx3')
    u = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    assert I.session_key([u], 'bx3', ('u8', True)) != I.session_key([u], 'bx3', ('u8', False)) != I.session_key([u], 'bx3')
    assert I.session_key([a.double()], 'bx3') != I.session_key([a], 'bx3')
    assert len({k, I.session_key([a, b], 'bx3')}) == 1                                  # hashable, equal keys collide


class _FakeWeight:
    def __init__(self, ptr, shape=(8, 8, 1, 1)):
        self.ptr, self.shape = ptr, shape

    def data_ptr(self):
        return self.ptr


@pytest.fixture
def fake_packs(monkeypatch):
    """kernels._packed_buffer / _pack_into without a device: every pack launch is recorded as (ptr, mode)"""
    launched = []
    monkeypatch.setattr(K, '_packed_buffer', lambda w, mode, math: K.PackedWeights(('buf', w.data_ptr(), mode), K.FMT_BX3))
    monkeypatch.setattr(K, '_pack_into', lambda w, mode, pw: launched.append((w.data_ptr(), mode)))
    return launched


def test_pack_plan_admit_set_never_records_an_outsider(fake_packs):
    plan = K.PackPlan(admit=[0x1000, 0x2000])
    plan.valid = True
    p1, p2, derived = _FakeWeight(0x1000), _FakeWeight(0x2000), _FakeWeight(0x9000)
    a = plan.lookup(p1, K.PACK_FWD, 'bx3')
    assert fake_packs == [(0x1000, K.PACK_FWD)] and len(plan.entries) == 1
    assert plan.lookup(p1, K.PACK_FWD, 'bx3') is a and len(fake_packs) == 1            # admitted: cached, no launch
    for n in range(1, 4):                                                              # an outsider: packed every time, never recorded
        d = plan.lookup(derived, K.PACK_FWD, 'bx3')
        assert d is not a and len(plan.entries) == 1 and fake_packs.count((0x9000, K.PACK_FWD)) == n
    assert all(key[0] in plan.admit for key in plan.entries)
    plan.lookup(p2, K.PACK_DGRAD_S1, 'bx3')
    plan.lookup(p1, K.PACK_FWD, 'hx2')                                                 # another arithmetic / mode: an entry of its own
    assert len(plan.entries) == 3
    # a recycled address: a NEW derived tensor at an address an earlier derived tensor had gets a fresh pack, not a cached one
    again = plan.lookup(_FakeWeight(0x9000), K.PACK_FWD, 'bx3')
    assert again is not d and fake_packs[-1] == (0x9000, K.PACK_FWD)
    # the unrestricted plan of the train step records everything, as before
    free = K.PackPlan()
    free.lookup(derived, K.PACK_FWD, 'bx3')
    assert free.admit is None and len(free.entries) == 1


class _Net(nn.Module):
    """a module that answers infer_spec() with a host-side forward (2 x + w)"""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.ones(1))
        self.calls = 0

    def infer_spec(self):
        def fwd(P, cfg, x, ref=None, keep=True):
            self.calls += 1
            assert keep is False and K._active_plan is not None and not torch.is_grad_enabled()
            return 2 * x + P['w'], None
        return fwd, ['w'], [self.w], {}


class _FakeGraph:
    def __init__(self, sess, ent):
        self.sess, self.ent, self.replayed = sess, ent, 0

    def replay(self):
        self.replayed += 1
        self.ent['out'] = self.sess._body(self.ent['inputs'], None)


@pytest.fixture
def host_session(monkeypatch):
    """InferenceSession with the device out of the way: the capture is a recorder whose `replay` recomputes from the static inputs"""
    monkeypatch.setattr(I, 'require_gpu', lambda t, what: None)
    captured = []

    def fake_capture(self, images, tag):
        del self.graphs.make_room()[:]
        ent = dict(inputs=[t.clone() for t in images], refs=[])
        ent['graph'] = _FakeGraph(self, ent)
        self.captures += 1
        captured.append(tuple(images[0].shape))
        return ent
    monkeypatch.setattr(I.InferenceSession, '_capture', fake_capture)
    return captured


def test_policy_eager_then_capture_then_replay_and_lru(host_session):
    net = _Net()
    sess = I.InferenceSession(net, max_graphs=2)
    assert sess.plan.admit == frozenset(I.pointer_tuple(net)) and sess.plan.valid
    x = torch.arange(4.).view(1, 1, 2, 2)
    out1 = sess(x)
    assert (sess.captures, sess.replays, net.calls) == (0, 0, 1)                       # call 1: eager
    out2 = sess(x)
    assert (sess.captures, sess.replays) == (1, 1)                                     # call 2: capture + replay
    out3 = sess(x + 1)
    assert (sess.captures, sess.replays) == (1, 2)                                     # call 3: replay, reading the new input
    assert torch.equal(out1, 2 * x + 1) and torch.equal(out2, out1) and torch.equal(out3, 2 * (x + 1) + 1)
    ent = sess.graphs.get(I.session_key([x], K.MATH))
    assert out3 is not ent['out'] and torch.equal(ent['inputs'][0], x + 1)             # a fresh tensor; inputs were copied in
    # three shapes through two slots: the least recently used goes, and comes back with a new capture (no second eager call)
    y, z = torch.zeros(1, 1, 3, 3), torch.zeros(1, 1, 4, 4)
    for t in (y, y, z, z):
        sess(t)
    assert host_session == [(1, 1, 2, 2), (1, 1, 3, 3), (1, 1, 4, 4)] and len(sess.graphs) == 2
    assert [k[0][0][0] for k in sess.graphs.keys()] == [(1, 1, 3, 3), (1, 1, 4, 4)]
    calls = net.calls
    assert torch.equal(sess(x), 2 * x + 1) and host_session[-1] == (1, 1, 2, 2) and net.calls == calls + 1
    assert [k[0][0][0] for k in sess.graphs.keys()] == [(1, 1, 4, 4), (1, 1, 2, 2)]
    sess.release()
    assert len(sess.graphs) == 0 and sess.plan is None
    with pytest.raises(RuntimeError, match='release'):
        sess(x)


def test_max_graphs_zero_is_packs_only(host_session):
    net = _Net()
    sess = I.InferenceSession(net, max_graphs=0)
    x = torch.ones(1, 1, 2, 2)
    for i in range(4):
        assert torch.equal(sess(x), 2 * x + 1)
    assert sess.captures == 0 and sess.replays == 0 and net.calls == 4 and host_session == [] and len(sess.graphs) == 0
    with pytest.raises(ValueError):
        I.InferenceSession(net, max_graphs=-1)
    with pytest.raises(TypeError, match='infer_spec'):
        I.InferenceSession(nn.Linear(2, 2))


def test_moved_parameters_and_another_arithmetic_rebuild(host_session):
    net = _Net()
    sess = I.InferenceSession(net, max_graphs=2)
    x = torch.ones(1, 1, 2, 2)
    sess(x), sess(x)
    assert sess.rebuilds == 1 and sess.captures == 1 and not sess.stale()
    plan = sess.plan
    with torch.no_grad():
        net.w.mul_(3.0)                                                                # in place: invisible (the caller's refresh())
    assert not sess.stale()
    sess.refresh()
    assert sess.rebuilds == 1 and sess.plan is plan and len(sess.graphs) == 1          # re-packed, graphs kept
    net.w = nn.Parameter(torch.full((1,), 5.0))                                        # re-assignment: another data_ptr
    assert sess.stale()
    out = sess(x)
    assert sess.rebuilds == 2 and sess.plan is not plan and len(sess.graphs) == 0 and torch.equal(out, 2 * x + 5)
    assert sess.plan.admit == frozenset(I.pointer_tuple(net))
    assert sess.captures == 1                                                          # (the shape starts over with an eager call)
    sess(x)
    assert sess.captures == 2
    prev = K.MATH
    try:
        K.set_math('f32' if prev != 'f32' else 'bx3')
        assert sess.stale()
        sess(x)
        assert sess.rebuilds == 3 and sess.math == K.MATH and len(sess.graphs) == 0
        K.set_math(prev)
        sess.refresh()                                                                 # refresh() notices it as well
        assert sess.rebuilds == 4 and sess.math == prev
    finally:
        K.set_math(prev)
