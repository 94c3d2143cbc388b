"""InferenceSession: one frozen network run over many images (validation every `val_freq` iterations, the `net(lq, ref)` loop of the
reference's scripts/eval/main_evaluation_*.py).  The no-gradient forward of the arch modules (nafnet_arch_utils.infer_fwd) packs every
weight afresh and issues every launch from the host on every call -- right between two optimiser steps, wasted on the second image of a
validation set.  A session packs the network's weights once and replays the forward of each input shape as a captured hipGraph.

    sess = InferenceSession(net, max_graphs=4)
    out = sess(lq, ref)            # the positional images of net.forward (NAFNetDynamicFusion: (lq, k_v)); bit-identical to it
    sess.refresh()                 # the weights changed in place: re-pack (one launch), keep the graphs
    sess.release()                 # drop graphs, their pool, the packs

The host-side bookkeeping (GraphLRU, session_key, what makes a session stale) needs no GPU and is tested without one."""
from collections import OrderedDict

import torch

from . import kernels as K
from .models.archs.nafnet_arch_utils import infer_spec, require_gpu


class GraphLRU:
    """the captured graphs of a session, least recently used first; at most `capacity` of them"""

    def __init__(self, capacity):
        self.capacity = int(capacity)
        self.items = OrderedDict()

    def get(self, key):
        e = self.items.get(key)
        if e is not None:
            self.items.move_to_end(key)
        return e

    def make_room(self):
        """-> the entries that have to go before one more is put (oldest first)"""
        out = []
        while self.items and len(self.items) >= self.capacity:
            out.append(self.items.popitem(last=False)[1])
        return out

    def put(self, key, entry):
        assert self.capacity > 0 and len(self.items) < self.capacity and key not in self.items
        self.items[key] = entry

    def keys(self):
        return list(self.items)

    def clear(self):
        self.items.clear()

    def __len__(self):
        return len(self.items)


def session_key(images, math, tag=None):
    """what a captured graph is valid for: the shape and dtype of every positional input (None for an absent one), the arithmetic
    (kernels.MATH) and the entry point (`tag`: None for __call__, ('u8', bgr) for run_u8)"""
    return (tuple(None if t is None else (tuple(t.shape), str(t.dtype)) for t in images), math, tag)


def pointer_tuple(net):
    """the addresses of the network's parameters and buffers: what a session can watch for `.to()` / re-assignment"""
    return tuple(t.data_ptr() for t in list(net.parameters()) + list(net.buffers()))


def tensor_slots(net):
    """where the parameters and buffers of `net` live: (owner's dict, key) per tensor, each tensor once, in pointer_tuple's order --
    parameters, then buffers.  Walking the module tree costs about a microsecond per module (1.2 ms for SFNet at num_res 16, on every
    call); looking the slots up again costs a dict access each and still sees what pointer_tuple sees: a tensor moved by `.to()`
    (same slot, other data_ptr) and a re-assigned one (same slot, other tensor)."""
    slots = []
    for attr in ('_parameters', '_buffers'):
        seen = set()
        for m in net.modules():
            d = getattr(m, attr)
            for k, t in d.items():
                if t is not None and id(t) not in seen:
                    seen.add(id(t))
                    slots.append((d, k))
    return slots


def slot_pointers(slots):
    """the data_ptr() of every slot, None once a slot is empty or gone (then nothing compares equal to it)"""
    try:
        return tuple(d[k].data_ptr() for d, k in slots)
    except (KeyError, AttributeError):
        return None


def clone_out(out):
    """a fresh copy of a captured entry's static output: one tensor, or a list of them (SFNet answers [out 1/4, out 1/2, out full]) ->
    a tensor / a list of fresh tensors"""
    if isinstance(out, (list, tuple)):
        return [t.clone() for t in out]
    return out.clone()


def full_size(out):
    """the output an image is written from: the tensor itself, or the last of a multi-scale list (the reference's validation reads preds[-1])"""
    return out[-1] if isinstance(out, (list, tuple)) else out


class InferenceSession:
    """`net`: any arch module routed through nafnet_arch_utils.infer_fwd (it answers infer_spec()).  `max_graphs`: how many captured
    forwards (one per input shapes / dtype / kernels.MATH) are kept, least recently used evicted first; 0 = packed weights only, every
    call eager.

    Per key the first call runs eagerly under the session's pack plan (the warm-up a capture needs: workspaces and tables are allocated
    outside it), the second captures and replays, later ones replay.  The result is always a fresh tensor -- for a network with a
    list-valued forward (SFNet: three scales) a list of fresh tensors; run_u8 converts the full-size one, the last.

    STALENESS IS THE CALLER'S BUSINESS.  The packs are made at construction and by refresh(), never in between: a session cannot see
    that a weight changed in place -- FusedClipAdamW and tdr_multi_ema write parameters through raw pointers, `tensor._version` does not
    move.  After an optimiser step, an EMA update, `load_state_dict`, `p.mul_()` ...: call refresh() before the next image, or the old
    packs answer -- under the current biases, norms and depthwise kernels, which are read in place: a mixture that is neither network.
    Only two things are noticed without it, at the next call: a parameter or buffer that moved (`.to()`, re-assignment: the tuple of
    data_ptr()s changed) and a change of kernels.MATH -- both drop packs and graphs and start over.

    The plan admits parameters and buffers of `net` only (kernels.PackPlan(admit=)): weights a forward derives per call are packed on
    the spot -- inside the graph once captured -- and never recorded, so `len(sess.plan.entries)` stops growing after the first call of a
    shape."""

    def __init__(self, net, max_graphs=4):
        if max_graphs < 0:
            raise ValueError('max_graphs must be >= 0')
        infer_spec(net)                          # (TypeError for a module that is not routed through infer_fwd)
        self.net, self.max_graphs = net, int(max_graphs)
        self.graphs = GraphLRU(self.max_graphs)
        self.warm = set()
        self.pool = None
        self.plan = None
        self.released = False
        self.captures = self.replays = self.rebuilds = 0
        self._build()

    # ---- weights
    def _build(self):
        self._drop_graphs()
        self.warm.clear()
        self.slots = tensor_slots(self.net)
        self.ptrs, self.math = slot_pointers(self.slots), K.MATH
        self.plan = K.PackPlan(admit=self.ptrs)
        self._repack()
        self.rebuilds += 1

    def _repack(self):
        self.plan.run()                          # one launch over every recorded weight (none yet at construction)
        self.plan.valid = True                   # whatever is recorded later is packed on the spot from the weights as they are

    def stale(self):
        """what the session can detect on its own: moved parameters / buffers, another arithmetic.  Checked on every call, so it reads the
        slots recorded by _build (tensor_slots) instead of walking the module tree again; a sub-module added or removed after
        construction is therefore not noticed -- build a new session for another network."""
        return slot_pointers(self.slots) != self.ptrs or K.MATH != self.math

    def refresh(self):
        """the weights changed in place: re-pack all of them (one multi-tensor launch).  Graphs stay -- they read the pack buffers."""
        self._alive()
        if self.stale():
            self._build()
        else:
            self._repack()

    def release(self):
        self._drop_graphs()
        self.warm.clear()
        self.plan = self.pool = None
        self.released = True

    def _alive(self):
        if self.released:
            raise RuntimeError('InferenceSession: used after release()')

    def _drop_graphs(self):
        if len(self.graphs) and torch.cuda.is_initialized():
            torch.cuda.synchronize()             # no replay in flight when the pool's memory goes back
        self.graphs.clear()
        self.pool = None

    # ---- forward
    def _forward(self, images):
        fwd, names, params, cfg = infer_spec(self.net)
        P = dict(zip(names, [p.detach() for p in params]))
        prev = K.set_pack_plan(self.plan)
        try:
            with torch.no_grad():
                return fwd(P, cfg, *[t if t is None else t.detach() for t in images], keep=False)[0]
        finally:
            K.set_pack_plan(prev)

    def _body(self, images, tag):
        if tag is None:
            return self._forward(images)
        bgr = tag[1]
        planes = [K.img_u8_to_planes(t, swap_rb=bgr) if t is not None and t.dtype == torch.uint8 else t for t in images]
        return K.planes_to_img_u8(full_size(self._forward(planes)).contiguous(), swap_rb=bgr)

    def _capture(self, images, tag):
        old = self.graphs.make_room()
        if old and torch.cuda.is_initialized():
            torch.cuda.synchronize()             # no replay in flight when an evicted graph's memory goes back to the pool
            del old
        if self.pool is None:
            self.pool = torch.cuda.graph_pool_handle()
        ent = dict(inputs=[None if t is None else t.clone() for t in images], refs=[], graph=torch.cuda.CUDAGraph())
        try:
            with K.workspace_capture(ent['refs']), torch.cuda.graph(ent['graph'], pool=self.pool, capture_error_mode='thread_local'):
                ent['out'] = self._body(ent['inputs'], tag)
        except RuntimeError as e:
            raise NotImplementedError(f'InferenceSession: the forward of {type(self.net).__name__} cannot be captured into a hipGraph -- '
                                      f'a host synchronisation stands in the way: {str(e).splitlines()[0]!r}; run it with '
                                      'max_graphs=0 (packed weights, eager launches)') from e
        self.captures += 1
        return ent

    def _run(self, images, tag):
        self._alive()
        if self.stale():
            self._build()
        require_gpu(images[0], type(self.net).__name__)
        images = [t if t is None else t.contiguous() for t in images]
        key = session_key(images, K.MATH, tag)
        if self.max_graphs == 0 or key not in self.warm:
            self.warm.add(key)
            return self._body(images, tag)
        ent = self.graphs.get(key)
        if ent is None:
            ent = self._capture(images, tag)
            self.graphs.put(key, ent)
        else:
            for dst, src in zip(ent['inputs'], images):
                if dst is not None:
                    dst.copy_(src, non_blocking=True)
        ent['graph'].replay()
        self.replays += 1
        return clone_out(ent['out'])             # the next replay overwrites the static output(s)

    def __call__(self, *images):
        return self._run(images, None)

    def run_u8(self, lq_u8, ref_u8=None, bgr=True):
        """bytes in -> bytes out on the device: lq_u8 / ref_u8 uint8 [N,H,W,C] as cv2 decodes them (`bgr`: channels 0 and 2 are exchanged
        on the way in and back, img2tensor(bgr2rgb=True) / tensor2img(rgb2bgr=True) of the reference) -> uint8 [N,H,W,C].  Both
        conversions (kernels.img_u8_to_planes / planes_to_img_u8) are part of the captured graph: one replay per image.  A second input
        that is not uint8 (the k_v of NAFNetDynamicFusion) is passed through as it is; None for an un-guided network."""
        images = (lq_u8,) if ref_u8 is None else (lq_u8, ref_u8)
        if lq_u8.dtype != torch.uint8:
            raise TypeError('run_u8: lq_u8 must be a uint8 [N,H,W,C] tensor')
        return self._run(images, ('u8', bool(bgr)))
