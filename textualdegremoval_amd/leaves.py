"""The deferred-leaf scheduler of the hand-written backward passes: which parameter-gradient launches wait, which of them share a
launch, on which stream they run, and in which order their gradients reach the collector.  Nothing here knows a network; the engines
issue leaves (leaf / leaf_fin / leaf_wgrad1x1) and mark where a pass starts, where a level ends and where the queue is run.

Weight gradients run on the side stream (kernels.on_side).  A backward helper called on its own joins the side branch before it returns
(its results are then ordinary current-stream tensors); inside a whole-network backward the joins are deferred to the end
(deferred_join / maybe_join) so the weight-gradient branch overlaps the data-gradient chain of later layers.

A LEAF is a parameter gradient nothing downstream in the backward reads (the NAFBlocks' conv1 / conv4 / conv5, a Restormer block's
pointwise convs, ...).  While a pass collects (`with collecting(...)`: the Pass object `current`; engine.late_leaves is the entry that
reads the engine's switches) leaves are queued instead of run, and run_late_leaves() runs them on a second HIP stream (kernels.lane)
next to the caller's remaining main chain: 1x1 weight gradients of one shape as ONE grouped launch (kernels.wgrad1x1_group), the small
finishing reductions as ONE table-driven launch per kind (kernels.*_multi).  In LEVEL mode (a data-parallel run, whose gradient buckets
are cut in arrival order) the queue is run at each level's end instead (level_end), on the current stream: no lane, no join.
Every grouped / table-driven launch of a pass takes the next `seq` number: the index of its pinned pointer table, recorded at warm-up
and replayed under graph capture -- the order of those launches is part of the contract.

RULE for queued leaves: a leaf reads its operands (`keep`, and whatever its closure names) when the queue is run -- after the whole main
backward chain.  Nothing may write those tensors in place (K.add_ and friends) or rebind the closure's names between queueing and the
run; every operand must be listed in `keep`.  engine.DEBUG_LEAVES = True checks the tensors' version counters at run time.
"""
import contextlib
from typing import Callable, NamedTuple, Optional

import torch

from . import kernels as K

_join_depth = 0         # open deferred_join blocks


class deferred_join:
    def __enter__(self):
        global _join_depth
        _join_depth += 1
        return self

    def __exit__(self, *exc):
        global _join_depth
        _join_depth -= 1
        if _join_depth == 0:
            K.side_join()
        return False


def maybe_join():
    if _join_depth == 0:
        K.side_join()


# ---- the three kinds of queue entry (`pre`: the prefix its gradient names get in the collector; `keep`: operands held until the join)
class Closure(NamedTuple):
    pre: str
    run: Callable                   # () -> {name: grad}
    keep: tuple


class Wgrad1x1(NamedTuple):
    pre: str
    key: tuple                      # kernels.wgrad1x1_group_key + (want_db,): requests of one key share a launch
    req: tuple                      # (x, dout, Cout, Cin, gate)
    want_db: bool
    post: Callable                  # (g, db) -> {name: grad}
    scp: Optional[tuple]            # (w, b, gamma, c_out, c, fmt): see leaf_wgrad1x1
    keep: tuple


class Finish(NamedTuple):
    pre: str
    names: tuple                    # the gradient names of what fin() returns
    fin: K.Finisher                 # kind, ws, dims; fin() is the single launch


class Pass:
    """the state of one collecting pass: the queue, the prefix leaves are queued under, the level mode, the number of grouped launches
    issued so far (`seq`), and the switches as they stood when the pass was entered"""

    def __init__(self, level=False, group=True, batch_finish=True, serial=False, debug=False):
        self.queue, self.pre, self.seq, self.stamps = [], '', 0, []
        self.level, self.group, self.batch_finish, self.serial, self.debug = level, group, batch_finish, serial, debug

    def put(self, entry, keep=()):
        if self.debug:              # (DEBUG_LEAVES: checked in _run)
            self.stamps += [(t, t._version) for t in keep if torch.is_tensor(t)]
        self.queue.append(entry)


current = None          # the Pass that collects leaves; None outside a pass, and once its queue has been handed to run_late_leaves


@contextlib.contextmanager
def collecting(on, **switches):
    """`with collecting(on, level=.., group=.., ...):` around a whole-network backward: leaves are queued until run_late_leaves()
    (level mode: until each level_end()); on=False, or weight gradients already on the side stream: nothing is queued"""
    global current
    current = Pass(**switches) if on and not K.SIDE_WGRAD else None
    try:
        yield current
    finally:
        current = None


def set_prefix(pre):
    """the prefix under which the leaves issued from here on are queued (their closures return names relative to it)"""
    if current is not None:
        current.pre = pre


def _hand_over(G, results):
    for pre, g in results:
        for k, v in g.items():
            G[pre + k] = v          # (item by item: a GradSink collector acts on __setitem__)


def leaf(keep, fn, G):
    """run a parameter-gradient leaf now (on the side stream), or queue it for the deferred pass.  fn() -> {name: grad}"""
    if current is not None:
        current.put(Closure(current.pre, fn, keep), keep)
        return
    with K.on_side(*keep):
        _hand_over(G, [('', fn())])


def leaf_fin(names, fin, G):
    """a leaf that reduces per-workgroup partials: fin() -> the gradients of `names`.  A kernels.Finisher with a `kind` is queued as
    such, so that _run can run all of one kind as one launch"""
    if current is not None and current.batch_finish and fin.kind is not None:
        current.put(Finish(current.pre, names, fin))
        return
    leaf((), lambda: dict(zip(names, fin())), G)


def leaf_wgrad1x1(keep, req, post, G, want_db=True, scp=None):
    """a leaf whose work is ONE 1x1 weight gradient (with the bias gradient unless want_db=False) -- req = (x, dout, Cout, Cin, gate) --
    followed by `post(g, db) -> {name: grad}` (db None without a bias): queued for the grouped launch when leaves are being collected and
    the shape qualifies, an ordinary leaf otherwise.
    scp = (w, b, gamma, c_out, c, fmt): `post` is fmt(*scaled_conv_param_grads(g.view(c_out, c), db, w, b, gamma)) (the NAFBlocks'
    conv5 / gamma), so that _run can run those of a pass as one launch"""
    x, dout, Cout, Cin, gate = req
    if current is not None and current.group:
        key = K.wgrad1x1_group_key(x, dout, Cout, Cin, gate)
        if key is not None:
            current.put(Wgrad1x1(current.pre, key + (want_db,), req, want_db, post, scp, keep), keep)
            return

    def run():
        r = K.conv_wgrad(x, dout, Cout, Cin, 1, gate=gate, want_db=want_db)
        return post(*K.side_keep(*r)) if want_db else post(K.side_keep(r), None)
    leaf(keep, run, G)


def _run(p, late, serial=False):
    """the queued leaves on lane 0 (the current stream if serial / SERIAL_LEAVES), 1x1 requests of one shape grouped -> [(prefix, grads)]"""
    with contextlib.nullcontext() if (p.serial or serial) else K.lane(0, sync=True):
        for t, v in p.stamps:
            assert t._version == v, 'a queued weight-gradient operand was modified in place before its deferred leaf ran'
        p.stamps = []
        groups, fins, outs = {}, {}, {}
        for i, e in enumerate(late):
            if isinstance(e, Wgrad1x1):
                groups.setdefault(e.key, []).append(i)
            elif isinstance(e, Finish):
                fins.setdefault(e.fin.kind, []).append(i)
        scp = []                                                 # posts that are a scaled_conv_param_grads call on a group's result
        for idxs in groups.values():                             # one launch + one reduction per shape
            res = K.wgrad1x1_group([late[i].req for i in idxs], seq=p.seq, want_db=late[idxs[0]].want_db)
            p.seq += 1
            for i, r in zip(idxs, res):
                if p.batch_finish and late[i].scp is not None:
                    scp.append((i, r))                           # one launch for all of them below
                else:
                    outs[i] = late[i].post(*r)
        if len(scp) > 1:
            items = []
            for i, (g5, s5) in scp:
                w5, b5, gam, c_out, c, _fmt = late[i].scp
                items.append((g5.view(c_out, c), s5, w5, b5, gam))
            for (i, _r), r3 in zip(scp, K.scaled_conv_param_grads_multi(items, seq=p.seq)):
                outs[i] = late[i].scp[5](*K.side_keep(*r3))
            p.seq += 1
        else:
            for i, r in scp:
                outs[i] = late[i].post(*r)
        for kind, idxs in fins.items():                          # finishing reductions: one table-driven launch per kind (shapes in the table)
            if len(idxs) == 1:
                outs[idxs[0]] = dict(zip(late[idxs[0]].names, late[idxs[0]].fin()))
                continue
            multi = K.pair_sum_partials_multi if kind == 'ln' else K.dw_param_finish_multi
            for i, r in zip(idxs, multi([(late[i].fin.ws,) + late[i].fin.dims for i in idxs], seq=p.seq)):
                outs[i] = dict(zip(late[i].names, r))
            p.seq += 1
        return [(e.pre, e.run() if isinstance(e, Closure) else outs[i]) for i, e in enumerate(late)]


def level_end(G):
    """level boundary of a backward pass that exchanges gradients: run what the level queued (grouped), hand its gradients over now"""
    p = current
    if p is None or not p.level or not p.queue:
        return
    late, p.queue = p.queue, []
    _hand_over(G, _run(p, late, serial=True))
    late.clear()


def run_late_leaves(G, main_chain):
    """deferred leaves on lane 0, `main_chain()` on the current stream, join, then hand the gradients to the collector in order.
    The pass stops collecting here: what main_chain() issues runs at once"""
    global current
    p = current
    if p is not None and p.level:   # gradient exchange: the remainder of the last level, then the main chain -- nothing runs beside it
        level_end(G)
    current = None
    if p is None or p.level or not p.queue:
        main_chain()
        return
    results = _run(p, p.queue)
    main_chain()
    K.lanes_join()
    _hand_over(G, results)
    p.queue.clear()     # (operands referenced until here: the allocator cannot recycle them under a running lane kernel)
