"""Host-side checks of SFNet's forward-only route (no GPU): how kernels.sf_region_chunks cuts a quadrant into row chunks, what
SFNet.infer_spec() hands a session, how a session copies a list-valued static output, and that the two entry points of the fused
GELU -> Gap / Patch_ap pair are declared, bound and exported."""
import os
import re

import pytest
import torch

from textualdegremoval_amd import inference as I
from textualdegremoval_amd import kernels as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(2, 2), (8, 12), (16, 24), (64, 80), (32, 48), (256, 256), (130, 6), (1024, 1024), (2048, 8), (6, 4096), (720, 1280)]


def covered(qh, rows, chunks):
    """the rows the kernels' chunk arithmetic visits: chunk j covers [j * rows, min((j + 1) * rows, qh))"""
    out = []
    for j in range(chunks):
        r0 = j * rows
        n = min(rows, qh - r0)
        assert n >= 1, 'an empty chunk'
        out += list(range(r0, r0 + n))
    return out


@pytest.mark.parametrize('H,W', SHAPES)
def test_chunks_cover_every_quadrant_row_exactly_once(H, W):
    rows, chunks = K.sf_region_chunks(H, W)
    assert covered(H // 2, rows, chunks) == list(range(H // 2))
    assert (rows, chunks) == K.sf_region_chunks(H, W) == K.sf_region_chunks(H, W, None)          # a pure function of (H, W)
    # a few thousand elements a workgroup, unless one row is already more (or the whole quadrant less)
    per = rows * (W // 2)
    assert per <= K.SF_REGION_CHUNK_ELEMS or rows == 1
    assert chunks == 1 or per * 2 > K.SF_REGION_CHUNK_ELEMS // 2 or rows == 1
    # evened out: the last chunk is short by less than one row per chunk
    assert rows * chunks - H // 2 < chunks


def test_override_is_honoured_and_the_last_chunk_may_be_ragged():
    assert K.sf_region_chunks(16, 24, 3) == (3, 3)                      # 8 quadrant rows: 3 + 3 + 2
    assert covered(8, 3, 3) == list(range(8))
    assert K.sf_region_chunks(16, 24, 1) == (1, 8)
    assert K.sf_region_chunks(16, 24, 8) == (8, 1) == K.sf_region_chunks(16, 24, 100)             # clamped to the quadrant
    assert K.sf_region_chunks(16, 24) == (8, 1)
    assert K.sf_region_chunks(256, 256) == (32, 4) and K.sf_region_chunks(64, 64) == (32, 1)
    for H, W in SHAPES:
        for r in (1, 2, 3, 5, 7, 64):
            rows, chunks = K.sf_region_chunks(H, W, r)
            assert rows == min(r, H // 2) and covered(H // 2, rows, chunks) == list(range(H // 2))
    for bad in [(7, 8), (8, 7), (0, 8)]:
        with pytest.raises(ValueError):
            K.sf_region_chunks(*bad)
    with pytest.raises(ValueError):
        K.sf_region_chunks(8, 8, 0)


def test_infer_spec_names_are_parameters_then_buffers_and_training_mode_raises():
    from textualdegremoval_amd.models.archs import define_network
    net = define_network(dict(type='SFNet', mode=['test', 'Outdoor'], num_res=1))
    with pytest.raises(ValueError, match='eval'):
        net.infer_spec()
    with pytest.raises(ValueError, match='eval'):
        I.InferenceSession(net)                                          # (raised before anything touches a device)
    net.eval()
    fwd, names, params, cfg = net.infer_spec()
    sd = list(net.state_dict())
    bufs = [k for k, _ in net.named_buffers()]
    assert bufs and names == [k for k in sd if k not in bufs] + [k for k in sd if k in bufs] and sorted(names) == sorted(sd)
    assert names[-len(bufs):] == bufs and all(k.endswith(('running_mean', 'running_var', 'num_batches_tracked')) for k in bufs)
    assert all(p is q for p, q in zip(params, list(net.parameters()) + list(net.buffers()))) and len(params) == len(names)
    assert tuple(p.data_ptr() for p in params) == I.pointer_tuple(net)   # what a session watches and its plan admits
    assert cfg == dict(num_res=1, tlsc=210) and callable(fwd)
    assert define_network(dict(type='SFNet', mode=['train', 'Indoor'], num_res=1)).eval().infer_spec()[3] == dict(num_res=1, tlsc=None)


def test_engine_switch_and_keep_rules():
    from textualdegremoval_amd import sfnet_engine as SE
    assert SE.INFER_KERNELS is True                                      # module switch (A/B in profiles/probe_sfnet_infer.py)
    with pytest.raises(ValueError, match='keep=False'):
        SE.net_fwd({}, torch.zeros(1, 3, 8, 8), 1, training=True, keep=False)
    with pytest.raises(ValueError):
        SE.net_fwd({}, torch.zeros(1, 3, 8, 8), 1, training=True, tlsc=246)
    with pytest.raises(ValueError, match='act=False'):               # (raised before any weight is looked up)
        SE.infer_conv(torch.zeros(1, 3, 8, 8), {}, 'x.', 3, act=True, res=torch.zeros(1, 3, 8, 8))


def test_staleness_check_reads_recorded_slots_and_sees_what_the_tree_walk_sees():
    from textualdegremoval_amd.models.archs import define_network
    net = define_network(dict(type='SFNet', mode=['train', 'Indoor'], num_res=1)).eval()
    slots = I.tensor_slots(net)
    assert I.slot_pointers(slots) == I.pointer_tuple(net)                # same tensors, same order: parameters, then buffers
    before = I.slot_pointers(slots)
    conv = net.Encoder[0].layers[0].conv1.main[0]
    with torch.no_grad():
        conv.weight.mul_(1.01)                                           # in place: invisible to both
    assert I.slot_pointers(slots) == before == I.pointer_tuple(net)
    conv.weight = torch.nn.Parameter(conv.weight.detach().clone())       # re-assigned: same slot, another tensor
    assert I.slot_pointers(slots) != before and I.slot_pointers(slots) == I.pointer_tuple(net)
    bn = net.Encoder[0].layers[0].dyna.bn
    bn.running_mean = bn.running_mean.clone()                            # a buffer too
    assert I.slot_pointers(slots) == I.pointer_tuple(net)
    del bn._buffers['running_var']
    assert I.slot_pointers(slots) is None                                # a slot that is gone compares unequal to everything
    shared = torch.nn.Linear(2, 2)
    two = torch.nn.Sequential(shared, shared)
    assert len(I.tensor_slots(two)) == 2 and I.slot_pointers(I.tensor_slots(two)) == I.pointer_tuple(two)      # shared tensors once


def test_clone_step_handles_tensor_and_list_outputs():
    a, b, c = torch.arange(4.), torch.arange(6.).view(2, 3), torch.ones(1)
    one = I.clone_out(a)
    assert isinstance(one, torch.Tensor) and torch.equal(one, a) and one.data_ptr() != a.data_ptr()
    for static in ([a, b, c], (a, b, c)):
        out = I.clone_out(static)
        assert isinstance(out, list) and len(out) == 3
        assert all(torch.equal(o, s) and o.data_ptr() != s.data_ptr() for o, s in zip(out, static))
    a.add_(1)                                                            # the next replay overwrites the static output, not the copy
    assert torch.equal(out[0], torch.arange(4.))
    assert I.full_size([a, b, c]) is c and I.full_size(a) is a


class _ListNet(torch.nn.Module):
    """answers infer_spec() with a host-side forward that returns three scales"""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))

    def infer_spec(self):
        def fwd(P, cfg, x, keep=True):
            assert keep is False
            return [x[..., ::4, ::4] + P['w'], x[..., ::2, ::2] + P['w'], x + P['w']], None
        return fwd, ['w'], [self.w], {}


def test_session_returns_fresh_lists_on_eager_and_replayed_calls(monkeypatch):
    monkeypatch.setattr(I, 'require_gpu', lambda t, what: None)

    class Graph:
        def __init__(self, sess, ent):
            self.sess, self.ent = sess, ent

        def replay(self):
            for dst, src in zip(self.ent['out'], self.sess._body(self.ent['inputs'], None)):
                dst.copy_(src)

    def fake_capture(self, images, tag):
        ent = dict(inputs=[t.clone() for t in images], refs=[])
        ent['out'] = [torch.full_like(t, float('nan')) for t in self._body(ent['inputs'], tag)]       # the static outputs
        ent['graph'] = Graph(self, ent)
        self.captures += 1
        return ent
    monkeypatch.setattr(I.InferenceSession, '_capture', fake_capture)
    sess = I.InferenceSession(_ListNet(), max_graphs=1)
    x = torch.arange(64.).view(1, 1, 8, 8)
    want = [x[..., ::4, ::4] + 1, x[..., ::2, ::2] + 1, x + 1]
    calls = [sess(x), sess(x), sess(x)]
    assert (sess.captures, sess.replays) == (1, 2)
    static = sess.graphs.get(I.session_key([x], K.MATH))['out']
    for out in calls:
        assert isinstance(out, list) and all(torch.equal(o, w) for o, w in zip(out, want))
    for out in calls[1:]:
        assert all(o.data_ptr() != s.data_ptr() for o, s in zip(out, static))
    later = sess(x + 1)
    assert torch.equal(later[2], x + 2) and torch.equal(calls[2][2], x + 1)        # an earlier result is not overwritten by a later replay


def test_entry_points_are_declared_bound_and_exported():
    from textualdegremoval_amd import _lib
    lib = _lib.load()
    txt = open(os.path.join(ROOT, 'include', 'tdr.h')).read()
    for sym in ('tdr_sf_act_region_sums', 'tdr_sf_act_region_apply'):
        assert re.search(r'^int ' + sym + r'\(', txt, re.M), sym
        assert sym in _lib.SIGNATURES and hasattr(lib, sym), sym
    assert len(_lib.SIGNATURES['tdr_sf_act_region_sums'][1]) == 10 and len(_lib.SIGNATURES['tdr_sf_act_region_apply'][1]) == 15
    # argument checks run before any launch: null pointers, odd sizes, a chunk count that does not cover the quadrant
    sums, apply_ = lib.tdr_sf_act_region_sums, lib.tdr_sf_act_region_apply
    assert sums(0, 1, 4, 8, 8, 4, 1, 1, 64, 0) != 0 and sums(64, 1, 4, 8, 8, 4, 1, 1, 0, 0) != 0
    for N, C, H, W, rows, chunks, act in [(1, 3, 8, 8, 4, 1, 1), (1, 4, 7, 8, 3, 1, 1), (1, 4, 8, 6 + 1, 4, 1, 0), (1, 4, 8, 8, 2, 1, 1),
                                          (1, 4, 8, 8, 2, 3, 1), (1, 4, 8, 8, 0, 1, 1), (1, 4, 8, 8, 4, 1, 2), (0, 4, 8, 8, 4, 1, 1)]:
        assert sums(64, N, C, H, W, rows, chunks, act, 64, 0) != 0, (N, C, H, W, rows, chunks, act)
        assert apply_(64, 64, 64, 64, 64, 64, N, C, H, W, rows, chunks, act, 64, 0) != 0
    assert apply_(64, 64, 64, 64, 64, 64, 1, 4, 8, 8, 4, 1, 1, 0, 0) != 0
    assert 'tdr_sf_act_region' in lib.tdr_last_error().decode()
