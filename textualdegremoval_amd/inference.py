"""InferenceSession: one frozen network run over many images (validation every `val_freq` iterations, the `net(lq, ref)` loop of the
reference's scripts/eval/main_evaluation_*.py).  The no-gradient forward of the arch modules (nafnet_arch_utils.infer_fwd) packs every
weight afresh and issues every launch from the host on every call -- right between two optimiser steps, wasted on the second image of a
validation set.  A session packs the network's weights once and replays the forward of each input shape as a captured hipGraph.

    sess = InferenceSession(net, max_graphs=4)
    out = sess(lq, ref)            # the positional images of net.forward (NAFNetDynamicFusion: (lq, k_v)); bit-identical to it
    sess.refresh()                 # the weights changed in place: re-pack (one launch), keep the graphs
    sess.release()                 # drop graphs, their pool, the packs
    out = sess.run_tiled(lq, ref, tile=256, overlap=32, tile_batch=4)      # an image of any size through the graph of ONE tile shape
    out = sess.run_tiled(lq, ref, tile=256, matcher=dino_matcher)          # ... every tile against its DINOv2-matched window of ref
    out = sess.run_ensemble(lq, ref, ops=8)                                # geometric self-ensemble: flips / transposes in, their mean out

The host-side bookkeeping (GraphLRU, session_key, what makes a session stale, the tile plan: tile_starts / tile_weights / tile_batches)
and the definition of the self-ensemble (dihedral / dihedral_inverse / ensemble_ops) need no GPU and are tested without one."""
from collections import OrderedDict

import numpy as np
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


# ---- the tile plan of run_tiled: where the tiles of one dimension start, how the tiles covering a pixel are weighted, how the tiles of
# a call are chunked into batches of one size
def tile_starts(L, tile, overlap):
    """the tiles of a dimension of length L -> (starts, t): t = min(tile, L) is their common length; one tile at 0 where L <= t, else
    0, s, 2s, ... (s = t - overlap) while i * s < L - t, then a last one clamped to the border at L - t"""
    L, tile, overlap = int(L), int(tile), int(overlap)
    if L <= 0 or tile <= 0 or overlap < 0 or overlap >= tile:
        raise ValueError(f'tile_starts: length {L}, tile {tile}, overlap {overlap} (want L > 0, tile > 0, 0 <= overlap < tile)')
    t = min(tile, L)
    if L <= t:
        return [0], t
    return list(range(0, L - t, t - overlap)) + [L - t], t


def tile_weights(L, tile, overlap):
    """the blend table of a dimension, a row per pixel y -> (first int32 [L], cnt int32 [L], w float32 [L, K]): the tiles covering y are
    first[y] ... first[y] + cnt[y] - 1 (always a contiguous range), w[y, a] the weight of the a-th of them, 0 for a >= cnt[y]; K = max cnt
    (not bounded by 2: the clamped last tile may lie over two others).  Tile i weighs r = min(j + 1, t - j, overlap + 1) at its offset
    j = y - starts[i] -- a ramp over the overlap, flat inside; normalised over the covering tiles in float64 (the sums are whole numbers),
    then cast: a pixel covered once weighs exactly 1.0f, and with overlap = 0 every weight is 1.0f"""
    starts, t = tile_starts(L, tile, overlap)
    j = np.arange(int(L), dtype=np.int64)[:, None] - np.asarray(starts, dtype=np.int64)[None, :]
    cover = (j >= 0) & (j < t)
    r = np.where(cover, np.minimum(np.minimum(j + 1, t - j), int(overlap) + 1), 0)
    first, cnt = cover.argmax(axis=1), cover.sum(axis=1)
    norm = r.astype(np.float64) / r.sum(axis=1, keepdims=True).astype(np.float64)
    w = np.zeros((int(L), int(cnt.max())), np.float32)
    for a in range(w.shape[1]):
        rows = np.nonzero(a < cnt)[0]
        w[rows, a] = norm[rows, first[rows] + a].astype(np.float32)
    return first.astype(np.int32), cnt.astype(np.int32), w


def tile_batches(n_tiles, tile_batch):
    """the tile indices 0 ... n_tiles - 1 (all images of a call: image-major, then row-major) in chunks of exactly `tile_batch`; the last
    chunk is padded by repeating its last tile, so every forward of a call -- and of every later image size -- has one shape"""
    n_tiles, tile_batch = int(n_tiles), int(tile_batch)
    if n_tiles <= 0 or tile_batch <= 0:
        raise ValueError(f'tile_batches: {n_tiles} tiles in batches of {tile_batch}')
    idx = list(range(n_tiles)) + [n_tiles - 1] * (-n_tiles % tile_batch)
    return [idx[k:k + tile_batch] for k in range(0, len(idx), tile_batch)]


# ---- the geometric self-ensemble of run_ensemble: the network on the 8 flips / transposes of an image, every answer transformed back, the
# mean of them (`test_x8` of KAIR, `self_ensemble` of BasicSR).  These functions are the definition -- the kernels (csrc/tdr_dihedral.hip)
# give their bits; they run on CPU tensors too.
def dihedral(x, op):
    """op code 0 ... 7 over the last two dimensions: bit 0 the horizontal flip (x -> W-1-x), bit 1 the vertical flip (y -> H-1-y), bit 2
    the transpose, applied after the flips.  Ops 0 - 3 keep the shape (the straight class), ops 4 - 7 answer (..., W, H) (the transposed
    class).  -> a view or a copy, not necessarily contiguous"""
    if op & 1:
        x = x.flip(-1)
    if op & 2:
        x = x.flip(-2)
    if op & 4:
        x = x.transpose(-2, -1)
    return x


def dihedral_inverse(y, op):
    """undoes dihedral(., op): the transpose first, then the flips"""
    if op & 4:
        y = y.transpose(-2, -1)
    if op & 2:
        y = y.flip(-2)
    if op & 1:
        y = y.flip(-1)
    return y


def ensemble_ops(spec):
    """which transforms a self-ensemble runs -> a sorted tuple of distinct op codes.  8 -> all of them, 4 -> the flips (0, 1, 2, 3), 2 ->
    (0, 1), 1 -> (0,) (the plain forward); an iterable of op codes is de-duplicated and sorted.  ValueError for anything else."""
    if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
        if int(spec) not in (1, 2, 4, 8):
            raise ValueError(f'ensemble_ops: {spec} transforms -- 8 (flips and transposes), 4 (flips), 2 (horizontal flip), 1 '
                             'or a list of op codes')
        return tuple(range(int(spec)))
    try:
        ops = list(spec)
    except TypeError:
        raise ValueError(f'ensemble_ops: {spec!r} is neither 1, 2, 4, 8 nor an iterable of op codes') from None
    if not ops or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < 8 for k in ops):
        raise ValueError(f'ensemble_ops: {spec!r} -- at least one op code, each an int in 0 ... 7')
    return tuple(sorted({int(k) for k in ops}))


def ensemble_classes(sel):
    """the selected ops by the shape they answer -> ((straight ops, transposed=False), (transposing ops, True))"""
    return (tuple(k for k in sel if k < 4), False), (tuple(k for k in sel if k >= 4), True)


def ensemble_inputs(src, extra, ops, swap_rb):
    """the inputs of one class's forward: the transforms `ops` of src and of every 4-D extra (the ref goes through the op its image goes
    through), op-major; any other extra (k_v [N,10,1024]) repeated op-major"""
    images = [K.dihedral_gather(src, ops, swap_rb=swap_rb)]
    for e in extra:
        if e is None or e.dim() != 4:
            images.append(e if e is None else e.repeat(len(ops), *([1] * (e.dim() - 1))))
        else:
            images.append(K.dihedral_gather(e.contiguous(), ops, swap_rb=swap_rb))
    return images


class TilePlan:
    """the device tables of one (N, H, W, tile, overlap, tile_batch): a single int32 buffer (one host-to-device copy), cut into the
    gather table [T', 3] of (n, y0, x0) per padded tile slot, the image index [T'] of every slot, and per dimension start [n], idx [L, 2]
    and the weights [L, K] (float32 bits)"""

    def __init__(self, N, H, W, tile, overlap, tile_batch, device):
        ys, self.th = tile_starts(H, tile[0], overlap)
        xs, self.tw = tile_starts(W, tile[1], overlap)
        self.ny, self.nx, self.n_tiles, self.tile_batch = len(ys), len(xs), N * len(ys) * len(xs), int(tile_batch)
        self.batches = tile_batches(self.n_tiles, tile_batch)
        slots = np.asarray(self.batches, dtype=np.int64).ravel()
        n, rem = slots // (self.ny * self.nx), slots % (self.ny * self.nx)
        table = np.stack([n, np.asarray(ys)[rem // self.nx], np.asarray(xs)[rem % self.nx]], axis=1).astype(np.int32)
        parts = [table.ravel(), n.astype(np.int32)]
        for L, starts, t in ((H, ys, tile[0]), (W, xs, tile[1])):    # (the tile as asked for: `overlap` may exceed a clamped one)
            first, cnt, w = tile_weights(L, t, overlap)
            parts += [np.asarray(starts, dtype=np.int32), np.stack([first, cnt], axis=1).ravel(), w.ravel().view(np.int32)]
        cuts = np.cumsum([0] + [p.size for p in parts])
        dev = torch.from_numpy(np.concatenate(parts)).to(device)
        cut = [dev[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
        self.table, self.image = cut[0].view(-1, 3), cut[1]
        self.ytabs = (cut[2], cut[3].view(H, 2), cut[4].view(torch.float32).view(H, -1))
        self.xtabs = (cut[5], cut[6].view(W, 2), cut[7].view(torch.float32).view(W, -1))


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
    shape.

    run_tiled / run_tiled_u8 cut images of any size into overlapping tiles of one size, run the tiles through the forward in batches of
    one size -- one key, one graph, whatever sizes follow -- and blend the tile outputs (see run_tiled).

    run_ensemble / run_ensemble_u8 (and `ensemble=` of the tiled calls) run the geometric self-ensemble: two small launches around
    forwards that go through the same ladder (see run_ensemble)."""

    TILE_PLANS = 32                              # device tables kept for repeated (N, H, W, tile, overlap, tile_batch)

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
        self.tile_plans = OrderedDict()
        self.last_match = None                   # what the matcher picked in the last run_tiled(..., matcher=) call
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
        self.tile_plans.clear()
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

    def _run(self, images, tag, take=None):
        """`take`: what becomes of the output instead of the default (the eager forward's own tensors / a clone of the captured entry's
        static ones): called with the output, its result returned -- run_tiled copies a replay's static output once, into the tile buffer"""
        self._alive()
        if self.stale():
            self._build()
        require_gpu(images[0], type(self.net).__name__)
        images = [t if t is None else t.contiguous() for t in images]
        key = session_key(images, K.MATH, tag)
        if self.max_graphs == 0 or key not in self.warm:
            self.warm.add(key)
            out = self._body(images, tag)
            return out if take is None else take(out)
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
        return (clone_out if take is None else take)(ent['out'])      # the next replay overwrites the static output(s)

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

    # ---- self-ensemble
    def _ensemble(self, src, extra, ops, swap_rb, u8, forward):
        """`forward(images, transposed)` -> the float32 outputs [k * N, C_out, Ho, Wo] of one class's stack, a tensor the next forward
        does not overwrite"""
        self._alive()
        sel = ensemble_ops(ops)
        require_gpu(src, type(self.net).__name__)
        src = src.contiguous()
        N, (H, W) = src.shape[0], (src.shape[1:3] if src.dtype == torch.uint8 else src.shape[2:])
        outs = []
        for cls, transposed in ensemble_classes(sel):
            out = forward(ensemble_inputs(src, extra, cls, swap_rb), transposed) if cls else None
            want = (len(cls) * N, (W, H) if transposed else (H, W))
            if out is not None and (out.dim() != 4 or (out.shape[0], tuple(out.shape[2:])) != want):
                raise NotImplementedError(f'self-ensemble: {type(self.net).__name__} answers {tuple(out.shape)} to {want[0]} images of '
                                          f'{want[1][0]} x {want[1][1]}; only networks of scale 1 are averaged')
            outs.append(out)
        return K.dihedral_mean(outs[0], outs[1], sel, N, u8=u8, swap_rb=swap_rb)

    def _ensemble_forward(self, images, transposed):
        # (a copy: the other class may replay the same graph and overwrite its static output)
        return self._run(tuple(images), None, lambda out: full_size(out).clone(memory_format=torch.contiguous_format))

    def run_ensemble(self, lq, *extra, ops=8):
        """geometric self-ensemble: lq float32 [N,C,H,W] -> float32 [N,C_out,H,W], the mean over the selected transforms of
        dihedral_inverse(net(dihedral(lq, op), ...), op) (`test_x8` of KAIR, `self_ensemble` of BasicSR).  `ops`: 8 (flips and transposes),
        4 (flips), 2 (horizontal flip), 1, or an iterable of op codes (ensemble_ops).

        The selected ops fall into two classes by the shape they give: straight (0 - 3: [.., H, W]) and transposed (4 - 7: [.., W, H]).
        Per class ONE launch (kernels.dihedral_gather) stacks the transforms of lq op-major -- and of every 4-D extra: the ref goes through
        the op its image goes through (MASA's geometry is symmetric under transposition, a transposed pair is valid whenever the original
        is); any other extra (k_v [N,10,1024]) is repeated op-major -- and ONE forward of len(class ops) * N images runs through the
        same pack plan and warm / capture / replay ladder as `sess(...)`, key (k * N, C, Ho, Wo): two keys, one for a square image whose
        classes hold equally many ops.  One more launch (kernels.dihedral_mean) transforms every answer back, adds them in ascending op
        order in fp32 and divides by their number.  A list-valued forward (SFNet) contributes its full-size output, the last.

        The limits of the network hold as they are, for the stacked batch and for the transposed shape (the 16 images of
        NAFNetDynamicFusion, width multiples): its error comes through.  ops=1 gives the bits of sess(lq, *extra).

        THE RESULT DEPENDS ON THE BATCH COMPOSITION as far as a sample's bits depend on its batch-mates: it is defined through the stacked
        forwards, not through eight separate ones."""
        if lq.dtype != torch.float32 or lq.dim() != 4:
            raise TypeError('run_ensemble: lq must be a float32 [N,C,H,W] tensor')
        return self._ensemble(lq, extra, ops, False, False, self._ensemble_forward)

    def run_ensemble_u8(self, lq_u8, ref_u8=None, bgr=True, ops=8):
        """run_ensemble on bytes: lq_u8 / ref_u8 uint8 [N,H,W,C] as cv2 decodes them -> uint8 [N,H,W,C].  The transforms are gathered
        straight from the bytes (converted as kernels.img_u8_to_planes converts, `bgr` exchanging channels 0 and 2 on the way in and back)
        and the mean writes the bytes itself, no float image in between: bit for bit
        planes_to_img_u8(run_ensemble(img_u8_to_planes(lq_u8), ...)), on the float call's keys and graphs -- the gather and the mean run
        eagerly around the replay, as in the tiled calls.  A second input that is not uint8 is passed on as in run_u8."""
        if lq_u8.dtype != torch.uint8 or lq_u8.dim() != 4:
            raise TypeError('run_ensemble_u8: lq_u8 must be a uint8 [N,H,W,C] tensor')
        return self._ensemble(lq_u8, () if ref_u8 is None else (ref_u8,), ops, bool(bgr), True, self._ensemble_forward)

    def _tiled_ensemble(self, src, extra, tile, overlap, tile_batch, swap_rb, u8, ops, matcher):
        if matcher is not None:
            raise NotImplementedError('run_tiled: a matcher together with ensemble= is not implemented (the matched window of a transformed '
                                      'tile is not the transformed window)')
        th, tw = (tile, tile) if isinstance(tile, int) else tile

        def forward(images, transposed):
            return self._tiled(images[0], tuple(images[1:]), (tw, th) if transposed else (th, tw), overlap, tile_batch, False)

        return self._ensemble(src, extra, ops, swap_rb, u8, forward)

    # ---- tiled
    def _tile_plan(self, N, H, W, tile, overlap, tile_batch, device):
        th, tw = (tile, tile) if isinstance(tile, int) else tile
        tile = (int(th), int(tw))
        key = (N, H, W, tile_starts(H, th, overlap)[1], tile_starts(W, tw, overlap)[1], int(overlap), int(tile_batch), str(device))
        plan = self.tile_plans.get(key)
        if plan is None:
            while len(self.tile_plans) >= self.TILE_PLANS:
                self.tile_plans.popitem(last=False)
            plan = self.tile_plans[key] = TilePlan(N, H, W, tile, int(overlap), int(tile_batch), device)
        else:
            self.tile_plans.move_to_end(key)
        return plan

    def _tiled(self, src, extra, tile, overlap, tile_batch, swap_rb, matcher=None):
        self._alive()
        require_gpu(src, type(self.net).__name__)
        src = src.contiguous()
        N, H, W = (src.shape[0], src.shape[1], src.shape[2]) if src.dtype == torch.uint8 else (src.shape[0], src.shape[2], src.shape[3])
        if matcher is not None:
            ref = extra[0] if extra else None
            if not torch.is_tensor(ref) or ref.dtype != torch.float32:
                raise TypeError('run_tiled: with a matcher the first extra input is the ref, a float32 [N,3,Hr,Wr] tensor')
            if ref.dim() != 4 or ref.shape[1] != 3:
                raise ValueError(f'run_tiled: with a matcher the first extra input is the ref [N,3,Hr,Wr], not {tuple(ref.shape)}')
        for e in extra:
            if e is not None and e.shape[0] != N:
                raise ValueError(f'run_tiled: an extra input of {e.shape[0]} rows for {N} images')
        plan = self._tile_plan(N, H, W, tile, overlap, tile_batch, src.device)
        B, held = plan.tile_batch, []
        bank = picked = None
        if matcher is not None:
            from .dino import window_grid
            if plan.th != plan.tw:
                raise NotImplementedError(f'run_tiled: the matcher unfolds square windows; tiles of {plan.th} x {plan.tw} are not matched')
            ref = ref.contiguous()
            grid = window_grid(ref.shape[2], ref.shape[3], plan.th)
            if tuple(ref.shape[2:]) != (plan.th, plan.tw):       # (else one window: top-1 of one candidate, the ref rows themselves)
                bank, picked = matcher.window_bank(ref, plan.th), []      # once per call, for every tile of every image

        def take(out):
            full = full_size(out)
            if full.dim() != 4 or tuple(full.shape[2:]) != (plan.th, plan.tw):
                raise NotImplementedError(f'run_tiled: {type(self.net).__name__} answers {tuple(full.shape)} to tiles of {plan.th} x {plan.tw}; '
                                          'only networks of scale 1 are tiled')
            if not held:
                held.append(torch.empty(plan.n_tiles, full.shape[1], plan.th, plan.tw, dtype=torch.float32, device=full.device))
            real = min(B, plan.n_tiles - k * B)                  # (the padding slots of the last batch are dropped)
            held[0][k * B:k * B + real].copy_(full[:real])

        for k in range(len(plan.batches)):
            tiles = K.tile_gather(src, plan.table[k * B:(k + 1) * B], plan.th, plan.tw, swap_rb=swap_rb)
            rows = plan.image[k * B:(k + 1) * B]
            others = tuple(e if e is None else e.index_select(0, rows) for e in (extra if bank is None else extra[1:]))
            if bank is not None:
                # the matcher runs eagerly in front of the replay: only the network's forward is captured, its key knows no ref size
                ref_in, index, corr = matcher.match_bank(tiles, bank, rows, ref)
                real = min(B, plan.n_tiles - k * B)
                picked.append((index[:real], corr[:real]))
                others = (ref_in,) + others
            self._run((tiles,) + others, None, take)
        if matcher is not None:
            if bank is None:
                index, corr = torch.zeros(plan.n_tiles, dtype=torch.int32, device=src.device), None
            else:
                index, corr = torch.cat([p[0] for p in picked]), torch.cat([p[1] for p in picked])
            self.last_match = dict(index=index, corr=corr, grid=grid)
        return K.tile_blend(held[0], N, H, W, plan.ytabs, plan.xtabs)

    def run_tiled(self, lq, *extra, tile=256, overlap=32, tile_batch=4, matcher=None, ensemble=None):
        """lq float32 [N,C,H,W] of ANY size -> float32 [N,C_out,H,W], through forwards of one shape: the image is cut into tiles of `tile`
        (an int or (th, tw); min(tile, image) per dimension) that overlap by `overlap` pixels, the last tile of a row / column clamped
        to the border (tile_starts); the tiles of all N images run through the network in batches of exactly `tile_batch` (the last batch
        padded with a repeated tile, tile_batches) -- every batch through the same pack plan and warm / capture / replay ladder as
        `sess(...)`, under ONE key (tile_batch, C, th, tw) whatever image sizes follow: one capture serves a validation folder of many
        sizes; with max_graphs=0 the batches run eagerly.  The outputs are blended with weights that ramp linearly over the overlap
        (tile_weights), one deterministic gather launch (kernels.tile_blend).

        `extra`: the other positional inputs of the network's forward -- ref [N,3,Hr,Wr] of the RefFusion classes, k_v [N,10,1024] of
        NAFNetDynamicFusion.  They are never tiled: row n accompanies every tile of image n (index_select, a copy).

        THE RESULT IS THE BLEND OF INDEPENDENT FORWARDS OF THE TILES, NOT THE FULL-FRAME FORWARD: whatever a block pools over the image
        (SCA, MDTA's channel attention, InstanceNorm) it pools per tile -- that is the point: a network trained on patches of `tile`
        sees the statistics it was trained on (`grids` / tile testing of the upstream NAFNet and Restormer test code).  It is the same
        computation as sess(lq), and gives its bits, only for tile >= image, tile_batch=1, N=1.  A list-valued forward (SFNet)
        contributes its full-size output, the last.  Scale-1 networks only (NotImplementedError otherwise).

        The device tables of a plan are kept per (N, H, W, th, tw, overlap, tile_batch) (the gather table holds the padding of the
        last batch, hence tile_batch), at most TILE_PLANS of them: a repeated image size copies nothing to the device.

        `matcher` (a dino.DinoMatcher): the first extra is the ref, float32 [N,3,Hr,Wr] of any size >= the tile, and every tile is
        restored against the (t, t) window of its image's ref that `matcher.match(tile, ref[n])` picks -- what the train step pairs a
        patch with -- instead of the whole ref.  The tokens of a ref's windows are computed once per call (matcher.window_bank), each
        batch of tiles costs one ViT pass over the tiles and one pass over the bank (matcher.match_bank), run eagerly in front of the
        replay: the captured forward sees (tile_batch, C, t, t) twice, ONE graph for every image size and every ref size.  Square
        tiles only (NotImplementedError otherwise, as match()).  A ref of exactly (t, t) has one window: no ViT pass, the bits of the
        call without a matcher.  Afterwards `sess.last_match` = dict(index int32 [n_tiles], corr float32 [n_tiles, Nw] (None in the
        one-window case), grid (ny, nx, stride)): device tensors, image-major then row-major like the tiles, padding slots dropped.

        `ensemble` (None, or what run_ensemble's `ops` takes): the self-ensemble of the tiled run -- by definition kernels.dihedral_mean
        over the two classes of run_tiled(the dihedral-gathered stack of len(class ops) * N images, the extras transformed as in
        run_ensemble, tile=(th, tw) -- (tw, th) for the transposed class), same overlap and tile_batch.  With square tiles one graph still
        serves every image size.  Not together with a matcher (NotImplementedError)."""
        if lq.dtype != torch.float32 or lq.dim() != 4:
            raise TypeError('run_tiled: lq must be a float32 [N,C,H,W] tensor')
        if ensemble is not None:
            return self._tiled_ensemble(lq, extra, tile, overlap, tile_batch, False, False, ensemble, matcher)
        return self._tiled(lq, extra, tile, overlap, tile_batch, False, matcher)

    def run_tiled_u8(self, lq_u8, extra=None, tile=256, overlap=32, tile_batch=4, bgr=True, matcher=None, ensemble=None):
        """run_tiled on bytes: lq_u8 uint8 [N,H,W,C] as cv2 decodes it -> uint8 [N,H,W,C].  The tiles are gathered straight from the bytes
        (converted as kernels.img_u8_to_planes converts, `bgr` exchanging channels 0 and 2 on the way in and back), the blended planes go
        through kernels.planes_to_img_u8: bit for bit planes_to_img_u8(run_tiled(img_u8_to_planes(lq_u8))), on the same graph.
        `extra`: None, one tensor or a sequence; a uint8 one (a ref image [N,Hr,Wr,3]) is converted once per call, not once per tile.
        `matcher`: as in run_tiled, the (converted) first extra being the ref.  `ensemble`: as in run_tiled; the transforms are gathered
        from the bytes and the mean writes the bytes (kernels.dihedral_mean(u8=True))."""
        if lq_u8.dtype != torch.uint8 or lq_u8.dim() != 4:
            raise TypeError('run_tiled_u8: lq_u8 must be a uint8 [N,H,W,C] tensor')
        extra = () if extra is None else (extra,) if torch.is_tensor(extra) else tuple(extra)
        extra = tuple(K.img_u8_to_planes(e.contiguous(), swap_rb=bgr) if e is not None and e.dtype == torch.uint8 else e for e in extra)
        if ensemble is not None:
            return self._tiled_ensemble(lq_u8, extra, tile, overlap, tile_batch, bool(bgr), True, ensemble, matcher)
        return K.planes_to_img_u8(self._tiled(lq_u8, extra, tile, overlap, tile_batch, bool(bgr), matcher), swap_rb=bgr)
