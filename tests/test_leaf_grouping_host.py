"""Host logic of the deferred-leaf scheduler (textualdegremoval_amd/leaves.py, entered through engine.late_leaves) without a GPU:
the kernel wrappers are replaced by CPU stand-ins that record what was asked of them.  Checked: leaves are queued only while a whole-network
backward collects them; 1x1 weight-gradient requests of one shape go out as ONE grouped call per shape (in first-seen order, with consecutive
table indices), the others as single calls; every gradient reaches the collector under its own prefix, in queue order; nothing is grouped when
the collector exchanges gradients (data-parallel run) or when grouping is switched off; finishing reductions and the conv5 / gamma posts of
a pass go out as one table-driven call per kind, with the next table indices; engine.DEBUG_LEAVES catches an operand written in place."""
import contextlib

import pytest
import torch

from textualdegremoval_amd import engine as E
from textualdegremoval_amd import leaves as L
from textualdegremoval_amd.kernels import Finisher


class _FakeK:
    SIDE_WGRAD = False

    def __init__(self):
        self.group_calls, self.single_calls, self.joins, self.multi_calls = [], [], 0, []

    # ---- what leaves.py calls
    def wgrad1x1_group_key(self, x, dout, Cout, Cin, gate):
        return None if Cin < 64 else (x.shape[0], Cin, Cout, x.shape[2], x.shape[3], int(gate))

    def wgrad1x1_group(self, reqs, seq=0, want_db=True):
        self.group_calls.append((seq, len(reqs), want_db, [r[0][0, 0, 0, 0].item() for r in reqs]))
        return [(torch.full((1, r[2], r[3], 1, 1), float(r[0][0, 0, 0, 0])), torch.zeros(r[2]) if want_db else None) for r in reqs]

    def conv_wgrad(self, x, dout, Cout, Cin, KH, gate=False, want_db=False, **kw):
        self.single_calls.append((Cout, Cin, float(x[0, 0, 0, 0])))
        g = torch.full((1, Cout, Cin, 1, 1), float(x[0, 0, 0, 0]))
        return (g, torch.zeros(Cout)) if want_db else g

    def pair_sum_partials_multi(self, items, seq=0):
        self.multi_calls.append(('ln', seq, [it[1:] for it in items]))
        return [(ws + 1, ws + 2) for ws, *_ in items]

    def dw_param_finish_multi(self, items, seq=0):
        self.multi_calls.append(('dw', seq, [it[1:] for it in items]))
        return [(ws + 1, ws + 2) for ws, *_ in items]

    def scaled_conv_param_grads_multi(self, items, seq=0):
        self.multi_calls.append(('scp', seq, [(tuple(g.shape), w, b, gam) for g, s, w, b, gam in items]))
        return [(g + 10, s, gam) for g, s, w, b, gam in items]

    def side_keep(self, *t):
        return t[0] if len(t) == 1 else t

    def lane(self, i, sync=False):
        return contextlib.nullcontext()

    def on_side(self, *keep):
        return contextlib.nullcontext()

    def lanes_join(self):
        self.joins += 1

    def side_join(self):
        pass


@pytest.fixture
def fake(monkeypatch):
    k = _FakeK()
    monkeypatch.setattr(L, 'K', k)
    monkeypatch.setattr(E, 'DEFER_WGRAD', True)
    monkeypatch.setattr(E, 'GROUP_LEAVES', True)
    return k


def _queue(G, tag, Cin, Cout, value, want_db=True):
    x = torch.full((2, Cin, 4, 8), float(value))
    d = torch.zeros(2, Cout, 4, 8)
    L.set_prefix(f'{tag}.')
    L.leaf_wgrad1x1((x, d), (x, d, Cout, Cin, False), lambda g, db: {'w': g, 'b': db} if want_db else {'w': g}, G, want_db=want_db)
    return x


def test_requests_of_one_shape_share_one_grouped_call(fake):
    G = {}
    with E.late_leaves(G):
        _queue(G, 'a', 128, 256, 1)
        _queue(G, 'b', 64, 128, 2)          # another shape: its own group
        _queue(G, 'c', 128, 256, 3)
        _queue(G, 'd', 32, 64, 4)           # not groupable (key None): an ordinary leaf
        _queue(G, 'e', 128, 256, 5, want_db=False)      # same channels, no bias gradient: a group of its own
        L.leaf((), lambda: {'ln': torch.ones(3)}, G)
        assert G == {} and len(L.current.queue) == 6    # nothing ran yet
        ran = []
        L.run_late_leaves(G, lambda: ran.append('main'))
    assert ran == ['main'] and fake.joins == 1 and L.current is None
    assert [(s, n, db) for s, n, db, _ in fake.group_calls] == [(0, 2, True), (1, 1, True), (2, 1, False)]
    assert fake.group_calls[0][3] == [1.0, 3.0]                         # the two 128 -> 256 requests, in queue order
    assert fake.single_calls == [(64, 32, 4.0)]
    assert set(G) == {'a.w', 'a.b', 'b.w', 'b.b', 'c.w', 'c.b', 'd.w', 'd.b', 'e.w', 'e.ln'}
    assert G['c.w'].flatten()[0].item() == 3.0 and G['e.w'].flatten()[0].item() == 5.0 and G['d.w'].flatten()[0].item() == 4.0


def test_nothing_is_deferred_or_grouped_with_a_gradient_exchange(fake):
    class Sink(dict):
        class reducer:
            collective = True
    G = Sink()
    with E.late_leaves(G):
        assert L.current is None
        _queue(G, 'a', 128, 256, 7)
        assert 'w' in G                                                 # ran at once (prefixes are the caller's business in this mode)
    assert fake.group_calls == [] and fake.single_calls == [(256, 128, 7.0)]


def test_grouping_switched_off_runs_single_launches_in_the_deferred_pass(fake, monkeypatch):
    monkeypatch.setattr(E, 'GROUP_LEAVES', False)
    G = {}
    with E.late_leaves(G):
        _queue(G, 'a', 128, 256, 1)
        _queue(G, 'b', 128, 256, 2)
        assert G == {}
        L.run_late_leaves(G, lambda: None)
    assert fake.group_calls == [] and [c[2] for c in fake.single_calls] == [1.0, 2.0]
    assert G['a.w'].flatten()[0].item() == 1.0 and G['b.w'].flatten()[0].item() == 2.0


def test_level_mode_groups_inside_a_data_parallel_backward(fake):
    """with a gradient exchange the leaves of a LEVEL are queued and run together at its end (level_end), on the current stream, and their
    gradients reach the collector right there -- before the next level starts -- so the buckets still fill in arrival order"""
    class Sink(dict):
        class reducer:
            collective = True
    G = Sink()
    with E.late_leaves(G, level_ok=True):
        assert L.current.queue == [] and L.current.level
        _queue(G, 'l3.a', 128, 256, 1)
        _queue(G, 'l3.b', 128, 256, 2)
        assert len(G) == 0
        L.level_end(G)
        assert set(G) == {'l3.a.w', 'l3.a.b', 'l3.b.w', 'l3.b.b'} and fake.group_calls == [(0, 2, True, [1.0, 2.0])]
        _queue(G, 'l2.a', 128, 256, 3)
        ran = []
        L.run_late_leaves(G, lambda: ran.append('main'))        # flushes the last level, then the main chain; no lane, no join
        assert ran == ['main'] and 'l2.a.w' in G and fake.joins == 0
    assert [c[0] for c in fake.group_calls] == [0, 1] and L.current is None


def _fin(kind, ws, dims, ran):
    """a finisher whose partials are the tensor `ws`: its own launch returns (ws - 1, ws - 2), the fake *_multi (ws + 1, ws + 2)"""
    return Finisher(kind, ws, dims, lambda: (ran.append((kind, dims)), (ws - 1, ws - 2))[1])


def _queue_finishers(G, ran):
    for tag, kind, v, dims in (('n0', 'ln', 10., (8, 64)), ('d0', 'dw', 20., (2, 64, 4, 8)), ('n1', 'ln', 30., (16, 32)),
                               ('d1', 'dw', 40., (2, 32, 8, 8)), ('d2', 'dw', 50., (2, 64, 4, 8)), ('big', None, 60., (4096, 64))):
        L.set_prefix(f'{tag}.')
        L.leaf_fin(('w', 'b'), _fin(kind, torch.tensor(v), dims, ran), G)


def test_finishing_reductions_of_one_kind_share_one_table_driven_call(fake, monkeypatch):
    """BATCH_FINISH: >= 2 queued finishers of a kind are ONE *_multi call (any mix of shapes), numbered after the groups in first-seen
    order of the kinds; a kind with a single entry, and a finisher without a kind, run their own closures"""
    G, ran = {}, []
    with E.late_leaves(G):
        _queue(G, 'a', 128, 256, 1)
        _queue_finishers(G, ran)
        L.set_prefix('solo.')
        L.leaf_fin(('w', 'b'), _fin('solo', torch.tensor(70.), (1,), ran), G)
        assert G == {} and ran == [] and len(L.current.queue) == 8
        assert [type(e) for e in L.current.queue] == [L.Wgrad1x1] + [L.Finish] * 5 + [L.Closure, L.Finish]
        L.run_late_leaves(G, lambda: None)
    assert [c[:2] for c in fake.group_calls] == [(0, 1)]
    assert fake.multi_calls == [('ln', 1, [(8, 64), (16, 32)]), ('dw', 2, [(2, 64, 4, 8), (2, 32, 8, 8), (2, 64, 4, 8)])]
    assert ran == [('solo', (1,)), (None, (4096, 64))]              # (the closure leaves run last, in queue order)
    assert list(G) == ['a.w', 'a.b'] + [f'{t}.{n}' for t in ('n0', 'd0', 'n1', 'd1', 'd2', 'big', 'solo') for n in 'wb']
    assert (G['n1.w'], G['n1.b'], G['d2.w'], G['solo.w'], G['big.b']) == (31., 32., 51., 69., 58.)
    # switched off: every finisher is an ordinary leaf
    monkeypatch.setattr(E, 'BATCH_FINISH', False)
    G2, ran, fake.multi_calls = {}, [], []
    with E.late_leaves(G2):
        _queue_finishers(G2, ran)
        assert all(type(e) is L.Closure for e in L.current.queue) and len(L.current.queue) == 6
        L.run_late_leaves(G2, lambda: None)
    assert fake.multi_calls == [] and [k for k, _ in ran] == ['ln', 'dw', 'ln', 'dw', 'dw', None]
    assert G2['n1.w'] == 29. and G2['d2.b'] == 48.


def _queue5(G, tag, value, own):
    """a conv5-like request: post is the single scaled_conv_param_grads launch (recorded in `own`), scp what the batched one needs"""
    x = torch.full((2, 128, 4, 8), float(value))
    d = torch.zeros(2, 64, 4, 8)
    L.set_prefix(f'{tag}.')
    L.leaf_wgrad1x1((x, d), (x, d, 64, 128, True), lambda g, db: (own.append(tag), {'w5': g.view(64, 128)})[1], G,
                    scp=(f'w.{tag}', f'b.{tag}', f'gamma.{tag}', 64, 128, lambda dw, db, dgam: {'w5': dw, 'gamma': dgam}))


def test_conv5_posts_behind_a_grouped_launch_share_one_call(fake):
    G, own = {}, []
    with E.late_leaves(G):
        _queue5(G, 'a', 1, own)
        _queue(G, 'x', 128, 256, 9)                                  # a group of another shape, without scp
        _queue5(G, 'b', 2, own)
        L.run_late_leaves(G, lambda: None)
    assert [c[:2] for c in fake.group_calls] == [(0, 2), (1, 1)] and own == []
    assert fake.multi_calls == [('scp', 2, [((64, 128), 'w.a', 'b.a', 'gamma.a'), ((64, 128), 'w.b', 'b.b', 'gamma.b')])]
    assert list(G) == ['a.w5', 'a.gamma', 'x.w', 'x.b', 'b.w5', 'b.gamma']
    assert G['b.w5'][0, 0].item() == 12.0 and G['a.gamma'] == 'gamma.a'
    # exactly one such request: its own post
    G, fake.multi_calls = {}, []
    with E.late_leaves(G):
        _queue5(G, 'a', 1, own)
        L.run_late_leaves(G, lambda: None)
    assert own == ['a'] and fake.multi_calls == [] and list(G) == ['a.w5'] and G['a.w5'][0, 0].item() == 1.0


@pytest.mark.parametrize('grouped', [False, True])
def test_debug_leaves_catches_an_operand_written_in_place(fake, monkeypatch, grouped):
    monkeypatch.setattr(E, 'DEBUG_LEAVES', True)
    G = {}
    with E.late_leaves(G):
        if grouped:
            x = _queue(G, 'a', 128, 256, 1)
            assert type(L.current.queue[0]) is L.Wgrad1x1
        else:
            x = torch.ones(4)
            L.leaf((x,), lambda: {'w': x * 2}, G)
        x.add_(1.0)
        with pytest.raises(AssertionError, match='modified in place'):
            L.run_late_leaves(G, lambda: None)
    assert G == {} and L.current is None
    with E.late_leaves(G):                                          # untouched operands pass
        x = _queue(G, 'a', 128, 256, 1) if grouped else torch.ones(4)
        L.leaf((x,), lambda: {'v': x * 2}, G)
        L.run_late_leaves(G, lambda: None)
    assert 'a.v' in G or 'v' in G
