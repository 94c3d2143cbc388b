"""Hand-written forward/backward of DRSformer-ref without the MEFC sub-network (`DRSformer200L_SPA_RefFusion`,
models/archs/network_drsformer_guided_arch_200L_SPA.py of the reference) on the HIP kernels -- SURVEY.md 8f, second "next"
architecture, and of the full `DRSformerRefFusion` / un-guided `DRSformer` with MEFC.  The network is restormer_engine's U-Net
walk (MASA front-end, dense convs, Down/Upsample, LayerNorm, fusion blocks) without the refinement blocks; the blocks differ:

* Top-K Sparse Attention (:257-328): the four masked softmaxes all multiply the same v, so they collapse into ONE c x c
  matrix A = sum_m attn_m * softmax(topk_m(logits)) (tdr_tksa_softmax) and the MDTA data flow is unchanged: q k^T as a
  per-image weight-gradient GEMM, A v and d[q;k] = W [q;k] as per-image 1x1 convs (tdr_tksa_bwd emits W, dtemperature, dattn_m).
* mixed-scale feed-forward (:213-253): 3x3 and 5x5 depthwise branches with ReLU, cross-concatenated, then the grouped
  2->1 convs (Conv2d(2h, h, groups=h)) with ReLU: tdr_dwk_fwd / tdr_dwk_bwd.

Reference defects (oracle/drsformer_ref_oracle.py): R1 (pyramid index), R5 (missing import, construction fails as shipped),
R6: the level-1 reference fusion is computed and discarded -- here it is not computed at all; `masa_blk_enc_level1.*` never
reach the engine (no gradient, as in the reference).
"""
import os

import torch

from . import engine as E
from . import kernels as K
from . import leaves as L
from . import restormer_engine as R


def _am(P):
    """attn1..attn4 as one [4] device vector"""
    am = torch.empty(4, dtype=torch.float32, device=P['attn.attn1'].device)
    for m in range(4):
        K.copy_rows(P[f'attn.attn{m + 1}'], 0, am[m:m + 1], 0, 1, 1)
    return am


def attn_fwd(xn, P, heads, res=None, keep=True):
    """Attention.forward (:274-328) on the normalised input; `res` is added to the projection (the block's skip).
    keep=False: (y, None); t goes after the depthwise conv, and the tail is restormer_engine.attn_tail_fwd's (project_out folded into
    the per-image weights)"""
    N, Cc, H, W = xn.shape
    t = R._pw_fwd(xn, P, 'attn.qkv')
    if not keep:
        xn = None
    qkv = K.dwconv_fwd(t, P['attn.qkv_dwconv.weight'], P.get('attn.qkv_dwconv.bias'))
    if not keep:
        t = None
    ss = K.row_sumsq(qkv, 2 * Cc)
    Gm = K.conv_wgrad(qkv[:, Cc:2 * Cc], qkv[:, :Cc], Cc, Cc, 1, per_image=True, fp16_range=True).view(N, Cc, Cc)
    am = _am(P)
    A, AT = K.tksa_softmax(Gm, ss, P['attn.temperature'], am, heads)
    y, o = R.attn_tail_fwd(qkv[:, 2 * Cc:], AT, P, heads, res, keep)
    return y, ((xn, t, qkv, ss, Gm, am, A, o) if keep else None)


def attn_bwd(dy, P, heads, saved, G):
    xn, t, qkv, ss, Gm, am, A, o = saved
    N, Cc, H, W = xn.shape
    do = R._pw_bwd(dy, o, P, 'attn.project_out', G)
    dA = K.conv_wgrad(qkv[:, 2 * Cc:], do, Cc, Cc, 1, per_image=True).view(N, Cc, Cc)
    Wm, G['attn.temperature'], dam = K.tksa_bwd(Gm, ss, P['attn.temperature'], am, dA, heads)
    for m in range(4):
        G[f'attn.attn{m + 1}'] = dam[m:m + 1]
    dqkv = torch.empty_like(qkv)
    R._img_conv(do, A, Cc, out=dqkv[:, 2 * Cc:])
    R._img_conv(qkv[:, :2 * Cc], Wm, 2 * Cc, out=dqkv[:, :2 * Cc])
    has_b = 'attn.qkv_dwconv.bias' in P
    dt, G['attn.qkv_dwconv.weight'], db = K.dwconv_bwd(dqkv, t, P['attn.qkv_dwconv.weight'], want_db=has_b)
    if has_b:
        G['attn.qkv_dwconv.bias'] = db
    return R._pw_bwd(dt, xn, P, 'attn.qkv', G)


def _split_ok(t2, h):
    """the in-place cross-concatenation needs 16-byte aligned plane slices and the 3x3 stencil route (W % 4 == 0)"""
    return t2.shape[-1] % 4 == 0 and (h * t2.shape[2] * t2.shape[3]) % 4 == 0 and not K.DWK_GENERIC and \
        os.environ.get('TDR_DWSG_TWO_PASS', '0') != '1'


def ffn_fwd(yn, P, res=None, keep=True):
    """FeedForward.forward (:240-253).  keep=False: (out, None); t2 goes after the first depthwise pair, x1 / x2 after the second"""
    t2 = R._pw_fwd(yn, P, 'ffn.project_in')                                         # [N, 2h, H, W]
    if not keep:
        yn = None
    h = t2.shape[1] // 2
    # x1 = [a3[:h] | a5[:h]], x2 = [a3[h:] | a5[h:]] (:244-247) are written in place: the 3x3 stencil owns the plane pair (c, c + h)
    # and stores its two planes to x1 / x2; the 5x5 conv runs per half.  a3 / a5 only exist as these slices.
    x1, x2 = torch.empty_like(t2), torch.empty_like(t2)
    w5, b5 = P['ffn.dwconv5x5.weight'], P.get('ffn.dwconv5x5.bias')
    if _split_ok(t2, h):
        a3 = K.dwk_fwd(t2, P['ffn.dwconv3x3.weight'], P.get('ffn.dwconv3x3.bias'), relu=True, out=(x1[:, :h], x2[:, :h]))
        K.dwk_fwd(t2[:, :h], w5[:h], None if b5 is None else b5[:h], relu=True, out=x1[:, h:])
        K.dwk_fwd(t2[:, h:], w5[h:], None if b5 is None else b5[h:], relu=True, out=x2[:, h:])
        a5 = (x1[:, h:], x2[:, h:])
    else:
        a3 = K.dwk_fwd(t2, P['ffn.dwconv3x3.weight'], P.get('ffn.dwconv3x3.bias'), relu=True)
        a5 = K.dwk_fwd(t2, w5, b5, relu=True)
        x1 = K.concat2(a3[:, :h], a5[:, :h])
        x2 = K.concat2(a3[:, h:], a5[:, h:])
    if not keep:
        N2, H2, W2, dev = t2.shape[0], t2.shape[2], t2.shape[3], t2.device
        t2 = a3 = a5 = None
        cat = torch.empty(N2, 2 * h, H2, W2, dtype=torch.float32, device=dev)
        K.dwk_fwd(x1, P['ffn.dwconv3x3_1.weight'], P.get('ffn.dwconv3x3_1.bias'), relu=True, out=cat[:, :h])
        x1 = None
        K.dwk_fwd(x2, P['ffn.dwconv5x5_1.weight'], P.get('ffn.dwconv5x5_1.bias'), relu=True, out=cat[:, h:])
        x2 = None
        return R._pw_fwd(cat, P, 'ffn.project_out', res=res), None
    cat = torch.empty(t2.shape[0], 2 * h, t2.shape[2], t2.shape[3], dtype=torch.float32, device=t2.device)
    z1 = K.dwk_fwd(x1, P['ffn.dwconv3x3_1.weight'], P.get('ffn.dwconv3x3_1.bias'), relu=True, out=cat[:, :h])   # straight into
    z2 = K.dwk_fwd(x2, P['ffn.dwconv5x5_1.weight'], P.get('ffn.dwconv5x5_1.bias'), relu=True, out=cat[:, h:])   # the concatenation
    out = R._pw_fwd(cat, P, 'ffn.project_out', res=res)
    return out, (yn, t2, a3, a5, x1, x2, z1, z2, cat)


def ffn_bwd(dout, P, saved, G):
    yn, t2, a3, a5, x1, x2, z1, z2, cat = saved
    h = t2.shape[1] // 2

    def put(name, dw, db):
        G[name + '.weight'] = dw
        if db is not None:
            G[name + '.bias'] = db
    dcat = R._pw_bwd(dout, cat, P, 'ffn.project_out', G)
    dx1, dw, db = K.dwk_bwd(dcat[:, :h], z1, x1, P['ffn.dwconv3x3_1.weight'], want_db='ffn.dwconv3x3_1.bias' in P)   # batch-strided
    put('ffn.dwconv3x3_1', dw, db)                                                                                      # views, no copies
    dx2, dw, db = K.dwk_bwd(dcat[:, h:], z2, x2, P['ffn.dwconv5x5_1.weight'], want_db='ffn.dwconv5x5_1.bias' in P)
    put('ffn.dwconv5x5_1', dw, db)
    w5 = P['ffn.dwconv5x5.weight']
    if isinstance(a3, tuple):
        # da3 = [dx1[:h] | dx2[:h]], da5 = [dx1[h:] | dx2[h:]] are read where they are (split halves / channel slices)
        dt2, dw, db = K.dwk_bwd((dx1[:, :h], dx2[:, :h]), a3, t2, P['ffn.dwconv3x3.weight'], want_db='ffn.dwconv3x3.bias' in P)
        put('ffn.dwconv3x3', dw, db)
        has_b = 'ffn.dwconv5x5.bias' in P
        dw5 = torch.empty_like(w5)
        db5 = torch.empty(2 * h, dtype=torch.float32, device=t2.device) if has_b else None
        # the 5x5 branch adds its input gradient onto the 3x3 branch's inside the kernel
        K.dwk_bwd(dx1[:, h:], a5[0], t2[:, :h], w5[:h], want_db=has_b, dx_out=dt2[:, :h], dw_out=dw5[:h],
                  db_out=None if db5 is None else db5[:h], accumulate=True)
        K.dwk_bwd(dx2[:, h:], a5[1], t2[:, h:], w5[h:], want_db=has_b, dx_out=dt2[:, h:], dw_out=dw5[h:],
                  db_out=None if db5 is None else db5[h:], accumulate=True)
        put('ffn.dwconv5x5', dw5, db5)
        return R._pw_bwd(dt2, yn, P, 'ffn.project_in', G)
    else:
        da3 = K.concat2(dx1[:, :h], dx2[:, :h])
        da5 = K.concat2(dx1[:, h:], dx2[:, h:])
        dt2, dw, db = K.dwk_bwd(da3, a3, t2, P['ffn.dwconv3x3.weight'], want_db='ffn.dwconv3x3.bias' in P)
        put('ffn.dwconv3x3', dw, db)
        dt2b, dw, db = K.dwk_bwd(da5, a5, t2, w5, want_db='ffn.dwconv5x5.bias' in P)
        put('ffn.dwconv5x5', dw, db)
    return R._pw_bwd(K.add_(dt2, dt2b), yn, P, 'ffn.project_in', G)


def tblock_fwd(x, P, heads, ln_type, keep=True):
    if not keep:                       # (out, None): the normalised tensors belong to attn_fwd / ffn_fwd, which let them go
        y, _ = attn_fwd(R._ln_fwd(x, P, 'norm1.', ln_type)[0], P, heads, res=x, keep=False)
        out, _ = ffn_fwd(R._ln_fwd(y, P, 'norm2.', ln_type)[0], P, res=y, keep=False)
        return out, None
    xn, mu1, rs1 = R._ln_fwd(x, P, 'norm1.', ln_type)
    y, sv_a = attn_fwd(xn, P, heads, res=x)
    yn, mu2, rs2 = R._ln_fwd(y, P, 'norm2.', ln_type)
    out, sv_f = ffn_fwd(yn, P, res=y)
    return out, (x, mu1, rs1, sv_a, y, mu2, rs2, sv_f)


def tblock_bwd(dout, P, heads, ln_type, saved):
    x, mu1, rs1, sv_a, y, mu2, rs2, sv_f = saved
    G = {}
    dyn = ffn_bwd(dout, P, sv_f, G)
    dy = R._ln_bwd(dyn, y, mu2, rs2, P, 'norm2.', ln_type, G, add=dout)
    dxn = attn_bwd(dy, P, heads, sv_a, G)
    dx = R._ln_bwd(dxn, x, mu1, rs1, P, 'norm1.', ln_type, G, add=dy)
    L.maybe_join()
    return dx, G


# ---------------------------------------------------------------------------
# whole network: restormer_engine's walk with these blocks, no refinement blocks; MEFC sub-networks after the patch embedding and
# after decoder_level1 in DRSformerRefFusion / DRSformer (cfg['mefc']), none in DRSformer200L_SPA_RefFusion
# ---------------------------------------------------------------------------
def _stage(fn, pre):
    """mefc_fwd / mefc_bwd on the sub-network `pre` as a stage of the walk (restormer_engine.walk_fwd / walk_bwd)"""
    return lambda x, P, cfg, *rest, **kw: fn(x, P, pre, *rest, **kw)


def net_fwd(P, cfg, inp, ref, keep=True):
    """keep=False: (out, None), nothing kept for a backward pass (restormer_engine.walk_fwd).  ref = None: the UN-GUIDED `DRSformer` of the same file (network_drsformer_guided_arch.py:586-676): no MASA pyramid, no
    fusion blocks, no padding (its PixelUnshuffle raises on sizes that are not multiples of 8), MEFC sub-networks always."""
    full = bool(cfg.get('mefc'))       # DRSformerRefFusion: MEFC sub-networks + a working level-1 fusion; else the 200L_SPA class
    return R.walk_fwd(P, cfg, inp, ref, 'DRSformer: H, W must be multiples of 8 (three PixelUnshuffle(2) stages); got {}x{}', tblock_fwd,
                      fuse=range(4) if full else range(1, 4),       # R6 (200L_SPA): the level-1 fusion is discarded; not computed here
                      head=_stage(mefc_fwd, 'encoder_level0.') if full else None, tail=_stage(mefc_fwd, 'refinement.') if full else None, keep=keep)


def net_bwd(dout, P, cfg, saved, G=None):
    full = bool(cfg.get('mefc'))
    return R.walk_bwd(dout, P, cfg, saved, G, tblock_bwd,
                      head=_stage(mefc_bwd, 'encoder_level0.') if full else None, tail=_stage(mefc_bwd, 'refinement.') if full else None)


# ---------------------------------------------------------------------------
# MEFC sub-network (`subnet`, network_drsformer_guided_arch.py:522-548) of the full DRSformerRefFusion (:679-1123)
# ---------------------------------------------------------------------------
OPS = ('sep_conv_1x1', 'sep_conv_3x3', 'sep_conv_5x5', 'sep_conv_7x7', 'dil_conv_3x3', 'dil_conv_5x5', 'dil_conv_7x7', 'avg_pool_3x3')
STEPS = 4


def _pw(x, w, relu=False, out=None):
    wp, mp, *_ = K.pack_weights(w, R.PACK_FWD)
    return K.conv_forward(x, wp, mp, w.shape[0], 1, relu=relu, out=out)


def _op_fwd(x, P, pre, j):
    name = OPS[j]
    if name == 'avg_pool_3x3':
        return K.avgpool3(x), None
    if name.startswith('sep_conv'):
        a = K.dwk_fwd(x, P[pre + 'op.0.weight'])
        r = _pw(a, P[pre + 'op.1.weight'], relu=True)
        c = K.dwk_fwd(r, P[pre + 'op.3.weight'])
        return _pw(c, P[pre + 'op.4.weight']), (a, r, c)
    a = K.dwk_fwd(x, P[pre + 'op.0.weight'], dil=2)
    return _pw(a, P[pre + 'op.1.weight']), (a,)


def _op_bwd(do, x, P, pre, j, sv, G):
    name = OPS[j]
    if name == 'avg_pool_3x3':
        return K.avgpool3(do.contiguous(), adjoint=True)
    if name.startswith('sep_conv'):
        a, r, c = sv
        dc = R._pw_bwd(do, c, P, pre + 'op.4', G)
        dr, G[pre + 'op.3.weight'], _ = K.dwk_bwd(dc, None, r, P[pre + 'op.3.weight'])
        da = R._pw_bwd(K.relu_bwd(dr, r), a, P, pre + 'op.1', G)
        dx, G[pre + 'op.0.weight'], _ = K.dwk_bwd(da, None, x, P[pre + 'op.0.weight'])
        return dx
    a, = sv
    da = R._pw_bwd(do, a, P, pre + 'op.1', G)
    dx, G[pre + 'op.0.weight'], _ = K.dwk_bwd(da, None, x, P[pre + 'op.0.weight'], dil=2)
    return dx


def mefc_fwd(x, P, pre, keep=True):
    """x [N,C,H,W] -> subnet(x).  Gating: mean_hw -> Linear -> ReLU -> Linear -> softmax over the 8 operations of each step;
    the per-image operation weights scale the (saved, unscaled) operation outputs while they are copied into the concat.
    keep=False: (out, None); an operation's output goes once it is copied into the concat, a step's concat after its `_out` conv"""
    N, C, H, W = x.shape
    nops = len(OPS)
    emb = K.plane_mean(x)
    h1 = K.linear_small_fwd(emb, P[pre + 'layers.0.ca_fc.0.weight'], P[pre + 'layers.0.ca_fc.0.bias'], relu=True)
    lg = K.linear_small_fwd(h1, P[pre + 'layers.0.ca_fc.2.weight'], P[pre + 'layers.0.ca_fc.2.bias'])
    wts = K.softmax_rows(lg.view(N * STEPS, nops))                      # [(n, step), op]
    wflat = wts.view(-1)
    g = pre + 'layers.1.'
    s0 = _pw(x, P[g + 'preprocess.op.0.weight'], relu=True)
    steps = []
    for i in range(STEPS):
        cat = torch.empty(N, nops * C, H, W, dtype=torch.float32, device=x.device)
        ops = []
        for j in range(nops):
            o, sv = _op_fwd(s0, P, f'{g}_ops.{i}._ops.{j}.', j)
            K.scale_copy(o, wflat[i * nops + j:], STEPS * nops, cat[:, j * C:(j + 1) * C])
            if keep:
                ops.append((o, sv))
            o = sv = None
        t = _pw(cat, P[f'{g}_ops.{i}._out.0.weight'], relu=True)
        s1 = K.add_relu(t, s0)
        if keep:
            steps.append((s0, cat, t, s1, ops))
        s0, cat, t, s1 = s1, None, None, None
    return s0, ((x, emb, h1, wts, steps) if keep else None)


def mefc_bwd(dout, P, pre, saved, G):
    x, emb, h1, wts, steps = saved
    N, C, H, W = x.shape
    nops = len(OPS)
    g = pre + 'layers.1.'
    wflat = wts.view(-1)
    dwts = torch.empty_like(wts)
    dwflat = dwts.view(-1)
    d = dout.contiguous()
    for i in reversed(range(STEPS)):
        s0, cat, t, s1, ops = steps[i]
        d = K.relu_bwd(d, s1)                                           # relu(t + res)
        dt = K.relu_bwd(d, t)                                           # _out's ReLU
        dcat = R._pw_bwd(dt, cat, P, f'{g}_ops.{i}._out.0', G)
        ds0 = d                                                         # the `res` branch
        for j in range(nops):
            o, sv = ops[j]
            dsl = dcat[:, j * C:(j + 1) * C]
            K.rows_dot(dsl, o, dwflat[i * nops + j:], STEPS * nops)
            do = K.scale_copy(dsl, wflat[i * nops + j:], STEPS * nops, torch.empty(N, C, H, W, dtype=torch.float32, device=x.device))
            ds0 = K.add_(_op_bwd(do, s0, P, f'{g}_ops.{i}._ops.{j}.', j, sv, G), ds0)
        d = ds0
    dpre = K.relu_bwd(d, steps[0][0])
    dx = R._pw_bwd(dpre, x, P, g + 'preprocess.op.0', G)
    dlg = K.softmax_rows(wts, dy=dwts).view(N, STEPS * nops)
    dh1, G[pre + 'layers.0.ca_fc.2.weight'], G[pre + 'layers.0.ca_fc.2.bias'] = K.linear_small_bwd(dlg, None, h1, P[pre + 'layers.0.ca_fc.2.weight'])
    demb, G[pre + 'layers.0.ca_fc.0.weight'], G[pre + 'layers.0.ca_fc.0.bias'] = K.linear_small_bwd(dh1, h1, emb, P[pre + 'layers.0.ca_fc.0.weight'])
    L.maybe_join()
    return K.plane_add_(dx, demb, 1.0 / (H * W))
