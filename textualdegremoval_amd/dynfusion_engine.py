"""NAFNetDynamicFusion forward/backward on the HIP kernels (models/archs/network_nafnet_guided_diffir_arch.py:250-375, :445-544).

The U-Net is engine.walk_fwd / walk_bwd, called with this module's block sequence (_seq_fwd / _seq_bwd); what lives here is the block,
the projections and their table.  Every block is conditioned on the textual embedding k_v [N, 10, 1024]: per block of width c
the projections `kernel` (2c outputs), `sg1.kernel` (4c) and `sg2.kernel` (4c) of the flattened k_v give per-(image, channel) affines

    m = x a0 + b0 -> norm1 -> conv1 -> dw3x3 -> u = dw a1 + b1 ; g = u[:c] u[c:] -> SCA -> conv3 ; y = x + (.) beta
    v = conv4(norm2(y)) a2 + b2 ; h = v[:c] v[c:] -> conv5 ; out = y + (.) gamma

All projections of the network run as ONE launch (csrc/tdr_dynfusion.hip, tdr_kvproj_fwd) into one [N, sum 10c] tensor; the blocks
read their slices.  The blocks run the per-op launches of engine.naf_fwd / naf_bwd (the fused head / tail chains are not extended)
plus the modulation kernels.  sg2's gate is materialised (`h`) and conv5 runs ungated on it.  No ATen arithmetic runs on
the device: torch only allocates and views memory.

A forward pass no backward follows (keep=False: inference, validation) saves nothing, and where the fused chains are supported a block
is three launches + SCA (csrc/tdr_dyn_infer.hip: the forward-only head / stencil / tail with the three affines applied in registers,
DESIGN 5n).
"""
import torch

from . import engine as E
from . import kernels as K
from . import leaves as L
from .kernels import PACK_DGRAD_S1, PACK_FWD

KV_DIM = 10 * 1024          # in_features of every projection (`nn.Linear(10 * 1024, ., bias=False)`, :257, :305)
# keep=False runs the fused forward-only launches where they are supported; False: the per-op launches everywhere, their intermediates
# dropped as they go (the A/B of profiles/probe_dynfusion_infer.py, and the same bits as keep=True).  A module switch, no environment knob.
INFER_KERNELS = True


def block_prefixes(cfg):
    """the blocks in forward order, with their widths: [(prefix, c)]"""
    out, chan = [], cfg['width']
    for lvl, n in enumerate(cfg['enc_blk_nums']):
        out += [(f'encoders.{lvl}.layers.{j}.', chan) for j in range(n)]
        chan *= 2
    out += [(f'middle_blks.layers.{j}.', chan) for j in range(cfg['middle_blk_num'])]
    for lvl, n in enumerate(cfg['dec_blk_nums']):
        chan //= 2
        out += [(f'decoders.{lvl}.layers.{j}.', chan) for j in range(n)]
    return out


PROJ_SUFFIXES = ('kernel.0.weight', 'sg1.kernel.0.weight', 'sg2.kernel.0.weight')


def proj_names(pre):
    return tuple(pre + s for s in PROJ_SUFFIXES)


class ProjTable:
    """the segment table of tdr_kvproj_*: one row {W, col0, rows, tile0} per projection weight, in block order.
    offs[prefix] = the block's first column of the projection output ([a0 | b0 | a1 | b1 | a2 | b2] = c, c, 2c, 2c, 2c, 2c)."""

    def __init__(self, P, blocks, device):
        R = K._lib.load().tdr_kvproj_tile_rows()
        rows, self.offs, self.weights, self.shapes = [], {}, [], []
        col = tile = 0
        for pre, c in blocks:
            self.offs[pre] = col
            for name, n in zip(proj_names(pre), (2 * c, 4 * c, 4 * c)):
                w = P[name]
                assert w.shape == (n, KV_DIM) and w.is_contiguous() and w.dtype == torch.float32
                rows.append((w.data_ptr(), col, n, tile))
                self.weights.append(name)
                self.shapes.append(torch.Size((n, KV_DIM)))
                col += n
                tile += -(-n // R)
        self.ld, self.ntiles, self.nseg = col, tile, len(rows)
        self.tab = torch.tensor(rows, dtype=torch.int64).to(device)
        self.key = tuple(r[0] for r in rows)


_tables = {}


def proj_table(P, blocks, device):
    """blocks = [(prefix, c)]; cached per set of weight buffers (the optimiser updates them in place)"""
    names = [n for pre, _ in blocks for n in proj_names(pre)]
    key = (str(device),) + tuple(P[n].data_ptr() for n in names)
    t = _tables.get(key)
    if t is None:
        if len(_tables) > 64:
            _tables.clear()
        t = _tables[key] = ProjTable(P, blocks, device)
    return t


def proj_fwd(P, blocks, kvf):
    """every projection of `blocks` in one launch -> (table, Kt [N, sum 10c])"""
    tab = proj_table(P, blocks, kvf.device)
    if K._ws_capture_refs is not None:
        K._ws_capture_refs.append(tab)       # a captured forward addresses the device table: it lives as long as the graph, whatever the cache does
    return tab, K.kvproj_fwd(tab.tab, tab.nseg, tab.ntiles, kvf, tab.ld)


def proj_bwd(tab, kvf, dK, G, need_dkv):
    """every projection weight gradient in one launch (into G), then the gradient of k_v [N, 10240] when asked for"""
    grads = [torch.empty(sh, dtype=torch.float32, device=kvf.device) for sh in tab.shapes]
    gtab = torch.tensor([t.data_ptr() for t in grads], dtype=torch.int64).to(kvf.device)
    K.kvproj_wgrad(tab.tab, gtab, tab.nseg, tab.ntiles, kvf, dK)
    for n, t in zip(tab.weights, grads):
        G[n] = t
    return K.kvproj_dkv(tab.tab, tab.nseg, tab.ntiles, dK, kvf.shape[1]) if need_dkv else None


def _slices(Kt, off, c):
    """(a0, b0, a1, b1, a2, b2) row slices of one block"""
    return (Kt[:, off:off + c], Kt[:, off + c:off + 2 * c], Kt[:, off + 2 * c:off + 4 * c], Kt[:, off + 4 * c:off + 6 * c],
            Kt[:, off + 6 * c:off + 8 * c], Kt[:, off + 8 * c:off + 10 * c])


def _dyn_naf_infer(x, P, Kt, off):
    """the block in three fused forward-only launches + SCA (csrc/tdr_dyn_infer.hip); the caller has checked the shape"""
    c = x.shape[1]
    a0, b0, a1, b1, a2, b2 = _slices(Kt, off, c)
    w1p, w3p, w4p, w5p = (K.pack_weights(P[k], PACK_FWD)[0] for k in ('conv1.weight', 'conv3.weight', 'conv4.weight', 'conv5.weight'))
    t1 = K.dyn_head_infer(x, a0, b0, P['norm1.weight'], P['norm1.bias'], E.LN_EPS, w1p, P['conv1.bias'])
    g, pooled = K.dyn_dwsg_fwd(t1, P['conv2.weight'], P['conv2.bias'], a1, b1)
    t1 = None
    s = K.sca_fwd(pooled, P['sca.1.weight'], P['sca.1.bias'])
    return K.dyn_tail_infer(g, s, x, w3p, P['conv3.bias'], P['beta'].view(-1), P['norm2.weight'], P['norm2.bias'], E.LN_EPS, w4p,
                            P['conv4.bias'], a2, b2, w5p, P['conv5.bias'], P['gamma'].view(-1))


def infer_fused_ok(x):
    """the support of the fused forward-only block: that of the NAFBlock chains (c in {32, 64, 128, 256}, HW % 64 == 0, a split
    arithmetic), rows the stencil reads as float4, a dense input"""
    N, c, H, W = x.shape
    return K.naf_tail_supported(c, H * W) and W % 4 == 0 and N <= 16 and x.is_contiguous()


def dyn_naf_fwd(x, P, Kt, off, keep=True):
    """NAFBlock_DynamicFusion.forward (:350-375) on x [N,c,H,W] with the block's projection slices of Kt.
    keep=False: a forward pass no backward follows -> (out, None).  Supported shapes run three fused launches + SCA (INFER_KERNELS);
    every other shape runs the same per-op launches as keep=True (same bits) and drops each intermediate once its last consumer is
    enqueued, as engine.naf_fwd does."""
    N, c, H, W = x.shape
    if not keep and INFER_KERNELS and infer_fused_ok(x):
        return _dyn_naf_infer(x, P, Kt, off), None
    a0, b0, a1, b1, a2, b2 = _slices(Kt, off, c)
    xn, mu1, rs1 = K.modln_fwd(x, a0, b0, P['norm1.weight'], P['norm1.bias'], E.LN_EPS)
    wp, mp, *_ = K.pack_weights(P['conv1.weight'], PACK_FWD)
    t1 = K.conv_forward(xn, wp, mp, 2 * c, 1, bias=P['conv1.bias'])
    if not keep:
        xn = mu1 = rs1 = None
    d2 = K.dwk_fwd(t1, P['conv2.weight'], P['conv2.bias'])
    if not keep:
        t1 = None
    g, pooled = K.modgate_fwd(d2, a1, b1, want_pool=True)
    if not keep:
        d2 = None
    s = K.sca_fwd(pooled, P['sca.1.weight'], P['sca.1.bias'])
    wp, mp, *_ = K.pack_weights(P['conv3.weight'], PACK_FWD)
    y = K.conv_forward(g, wp, mp, c, 1, kscale=s, bias=P['conv3.bias'], scale=P['beta'].view(-1), res=x)
    if not keep:
        g = None
    yn, mu2, rs2 = K.layernorm2d_fwd(y, P['norm2.weight'], P['norm2.bias'], E.LN_EPS)
    wp, mp, *_ = K.pack_weights(P['conv4.weight'], PACK_FWD)
    t4 = K.conv_forward(yn, wp, mp, 2 * c, 1, bias=P['conv4.bias'])
    if not keep:
        yn = mu2 = rs2 = None
    h, _ = K.modgate_fwd(t4, a2, b2)
    if not keep:
        t4 = None
    wp, mp, *_ = K.pack_weights(P['conv5.weight'], PACK_FWD)
    out = K.conv_forward(h, wp, mp, c, 1, bias=P['conv5.bias'], scale=P['gamma'].view(-1), res=y)
    if not keep:
        return out, None
    return out, (x, xn, mu1, rs1, t1, d2, g, pooled, s, y, yn, mu2, rs2, t4, h, off)


def dyn_naf_bwd(dout, P, saved, Kt, dK):
    """-> (dx, G); the gradients of the block's projection outputs go to its columns of dK"""
    x, xn, mu1, rs1, t1, d2, g, pooled, s, y, yn, mu2, rs2, t4, h, off = saved
    N, c, H, W = x.shape
    a0, b0, a1, b1, a2, b2 = _slices(Kt, off, c)
    da0, db0, da1, db1, da2, db2 = _slices(dK, off, c)
    beta, gamma = P['beta'].view(-1), P['gamma'].view(-1)
    G = {}
    dout = dout.contiguous()
    # ---- conv5 (+ gamma) on the materialised gate h
    G5, S5 = K.conv_wgrad(h, dout, c, c, 1, want_db=True)
    dw5, db5, dgam = K.scaled_conv_param_grads(G5.view(c, c), S5, P['conv5.weight'], P['conv5.bias'], gamma)
    G['conv5.weight'], G['conv5.bias'], G['gamma'] = dw5.view(c, c, 1, 1), db5, dgam.view(1, c, 1, 1)
    wp, mp, *_ = K.pack_weights(P['conv5.weight'], PACK_DGRAD_S1)
    dh = K.conv_forward(dout, wp, mp, c, 1, kscale=gamma)
    # ---- sg2 -> conv4 -> norm2 (+ the residual branch of `y + x * gamma`)
    dt4 = K.modgate_bwd(dh, t4, a2, b2, da2, db2)
    g4, b4 = K.conv_wgrad(yn, dt4, 2 * c, c, 1, want_db=True)
    G['conv4.weight'], G['conv4.bias'] = g4.view(2 * c, c, 1, 1), b4
    wp, mp, *_ = K.pack_weights(P['conv4.weight'], PACK_DGRAD_S1)
    dyn = K.conv_forward(dt4, wp, mp, c, 1)
    dy, G['norm2.weight'], G['norm2.bias'] = K.layernorm2d_bwd(dyn, y, mu2, rs2, P['norm2.weight'], add=dout)
    # ---- conv3 / SCA / beta
    G3, S3 = K.conv_wgrad(g, dy, c, c, 1, per_image=True, want_db=True)
    dw3, db3, dbeta, dwsca, dbsca, dpooled = K.sca_bwd(G3, S3, P['conv3.weight'], P['conv3.bias'], beta, s, pooled, P['sca.1.weight'])
    G['conv3.weight'], G['conv3.bias'], G['beta'] = dw3, db3, dbeta
    G['sca.1.weight'], G['sca.1.bias'] = dwsca, dbsca
    wp, mp, *_ = K.pack_weights(P['conv3.weight'], PACK_DGRAD_S1)
    dg = K.conv_forward(dy, wp, mp, c, 1, kscale=beta, scale=s, bias2=dpooled, bias2_mul=1.0 / (H * W))
    # ---- sg1 -> depthwise conv2
    dd2 = K.modgate_bwd(dg, d2, a1, b1, da1, db1)
    dt1, G['conv2.weight'], G['conv2.bias'] = K.dwk_bwd(dd2, None, t1, P['conv2.weight'], want_db=True)
    # ---- conv1 -> norm1 (input recomputed) -> the modulation x a0 + b0 (+ dy)
    g1, b1g = K.conv_wgrad(xn, dt1, 2 * c, c, 1, want_db=True)
    G['conv1.weight'], G['conv1.bias'] = g1.view(2 * c, c, 1, 1), b1g
    wp, mp, *_ = K.pack_weights(P['conv1.weight'], PACK_DGRAD_S1)
    dxn = K.conv_forward(dt1, wp, mp, c, 1)
    m = K.nc_affine(x, a0, b0)
    dm, G['norm1.weight'], G['norm1.bias'] = K.layernorm2d_bwd(dxn, m, mu1, rs1, P['norm1.weight'])
    dx = K.nc_affine_bwd(dm, x, a0, da0, db0, add=dy)
    return dx, G


def _seq_fwd(x, P, pre, n, Kt, tab, keep=True):
    saved = []
    for i in range(n):
        bp = f'{pre}{i}.'
        x, sv = dyn_naf_fwd(x, E._sub(P, bp), Kt, tab.offs[bp], keep=keep)
        saved.append(sv)
    return x, (saved if keep else None)


def _seq_bwd(d, P, pre, n, saved, Kt, dK, G):
    for i in reversed(range(n)):
        bp = f'{pre}{i}.'
        d, g = dyn_naf_bwd(d, E._sub(P, bp), saved[i], Kt, dK)
        E._put(G, bp, g)
    return d


def flat_kv(kv, N):
    """k_v [N, 10, 1024] -> [N, 10240] (torch.flatten(k_v, start_dim=1), :353); a different feature count fails as the reference's
    Linear does (defect R10: a Mapper(num_words=20) embedding)"""
    kvf = kv.reshape(kv.shape[0], -1)
    if kvf.shape[1] != KV_DIM:
        raise RuntimeError(f'mat1 and mat2 shapes cannot be multiplied ({kvf.shape[0]}x{kvf.shape[1]} and {KV_DIM}x(.)): '
                           f'NAFNetDynamicFusion projects k_v flattened to 10 x 1024 features')
    if kvf.shape[0] != N:
        raise ValueError(f'k_v has batch {kvf.shape[0]}, the image batch is {N}')
    if N > 16:
        raise NotImplementedError('NAFNetDynamicFusion on the HIP path: at most 16 images per call (the projection kernels keep one '
                                  'accumulator per image)')
    return kvf.contiguous()


def dyn_unet_fwd(P, cfg, inp, kv, keep=True):
    """NAFNetDynamicFusion.forward (:512-536) -> (out, saved): engine.walk_fwd over the modulated blocks; saved = the walk's
    + (kvf, Kt, projection table).  keep=False: (out, None) -- the walk releases the skips behind their decoder level, the blocks save
    nothing (dyn_naf_fwd)."""
    kvf = flat_kv(kv, inp.shape[0])
    tab, Kt = proj_fwd(P, block_prefixes(cfg), kvf)
    out, saved = E.walk_fwd(P, cfg, inp, seq=lambda x, P, pre, n, keep=True: _seq_fwd(x, P, pre + 'layers.', n, Kt, tab, keep=keep),
                            keep=keep)
    return out, (saved + (kvf, Kt, tab) if keep else None)


def dyn_block_fwd(P, cfg, x, kv, keep=True):
    """one NAFBlock_DynamicFusion with its own projection table (the module on its own) -> (out, saved); saved = (block's, table, kvf, Kt).
    cfg is unused (the signature of the whole-network forwards)"""
    kvf = flat_kv(kv, x.shape[0])
    tab, Kt = proj_fwd(P, [('', x.shape[1])], kvf)
    out, saved = dyn_naf_fwd(x.contiguous(), P, Kt, 0, keep=keep)
    return out, ((saved, tab, kvf, Kt) if keep else None)


def dyn_unet_bwd(dout, P, cfg, saved, need_dkv=True, G=None):
    """-> (dinp, dkv or None, G, dK): gradients w.r.t. the image, k_v (shape [N, 10240]), every parameter, and the projection outputs"""
    kvf, Kt, tab = saved[-3:]
    dK = torch.empty_like(Kt)            # every column is written by exactly one block's reductions
    with L.deferred_join():              # (the walk's side branch is joined after the projection launches)
        dinp, G = E.walk_bwd(dout, P, cfg, saved, G,
                             seq=lambda d, P, pre, n, sv, G: _seq_bwd(d, P, pre + 'layers.', n, sv, Kt, dK, G))
        dkv = proj_bwd(tab, kvf, dK, G, need_dkv)
    return dinp, dkv, G, dK
