"""Hand-written forward/backward of Restormer-ref (models/archs/network_restormer_guided_arch.py of the
reference) on the HIP kernels -- SURVEY.md 8a rows a13-a18 -- and the U-Net walk of the whole Restormer family.

Same conventions as engine.py (whose MASA front-end, dense-conv helpers and encoder this reuses): `*_fwd`
returns (out, saved), `*_bwd` returns (dx, grads); parameters travel as dicts keyed by the reference's
state-dict names.  No ATen arithmetic runs on the device: every tensor op is a call into libtdr_hip.so.

walk_fwd / walk_bwd run the 4-level U-Net that RestormerRefFusion, PromptIR(-ref) and DRSformer(-ref) share, guided
or un-guided: patch embed, encoder levels with optional MASA fusion stages and Downsample, Upsample + concat +
reduce_chan_level* + decoder levels, output conv.  promptir_engine and drsformer_engine pass in their own blocks and
stages (the transformer block pair, a stage before each Upsample, stages after the patch embedding and after
decoder_level1); net_fwd / net_bwd here are Restormer's call.

Reference defect R1: `RestormerRefFusion.forward` indexes the 4-level encoder pyramid one slot off (feat[4]
of a 4-entry list, :790-793,832-846).  The only assignment under which that code runs is feat[k] = L_k;
this engine uses [L1..L4] with padder_size 8 (:546), exactly what the golden generator's wrapped Encoder does.

MDTA (:246-277) on this hardware: the "tokens" are channels, so both contractions over the H*W pixels are
convolution-shaped -- q k^T is a per-image weight-gradient GEMM (tdr_conv_wgrad, per_image), attn v is a 1x1
convolution with per-image weights -- and run on the MFMA kernels; csrc/tdr_mdta.hip does the c x c softmax
algebra and emits the weights already in the packed layout those kernels read.
"""
import contextlib
import types

import torch

from . import engine as E
from . import kernels as K
from . import leaves as L
from .kernels import EPI_PSHUF, PACK_DGRAD_S1, PACK_FWD

LN_EPS = 1e-5        # :190,208
PADDER_LOG2 = 3      # self.padder_size = 2 ** 3 (:546)
# a forward pass that keeps nothing (keep=False) folds attn.project_out into the per-image attention weights (kernels.attn_fold_proj):
# Wo (A v) = (Wo A) v, one 1x1 convolution and no `o` plane; False: the unfolded launches of the training forward, `o` dropped after
# project_out -- the bits of keep=True (module switch for A/B runs, profiles/probe_restormer_infer.py; not an environment knob)
INFER_FOLD = True


# ---------------------------------------------------------------------------
# small helpers
# ---------------------------------------------------------------------------
def _kw(keep):
    """what a stage callable is called with: nothing more than before when everything is kept, `keep=False` otherwise"""
    return {} if keep else {'keep': False}


def _ln_fwd(x, P, pre, ln_type):
    """LayerNorm (:211-218): BiasFree (:172-190) scales the uncentred x; WithBias (:193-208)."""
    center = ln_type != 'BiasFree'
    return K.layernorm2d_fwd(x, P[pre + 'body.weight'], P[pre + 'body.bias'] if center else None, LN_EPS, center=center)


def _ln_bwd(go, x, mu, rs, P, pre, ln_type, G, add=None):
    center = ln_type != 'BiasFree'
    gx, gw, gb = K.layernorm2d_bwd(go, x, mu, rs, P[pre + 'body.weight'], add=add, center=center)
    G[pre + 'body.weight'] = gw
    if center:
        G[pre + 'body.bias'] = gb
    return gx


def _pw_fwd(x, P, name, res=None):
    """1x1 conv `name` (bias optional)."""
    w = P[name + '.weight']
    wp, mp, *_ = K.pack_weights(w, PACK_FWD)
    return K.conv_forward(x, wp, mp, w.shape[0], 1, bias=P.get(name + '.bias'), res=res)


def _pw_bwd(dout, x, P, name, G):
    """returns dx; stores dW (and db)."""
    w = P[name + '.weight']
    Cout, Cin = w.shape[0], w.shape[1]
    has_b = (name + '.bias') in P
    # parameter gradient: a leaf off the data-gradient chain (leaves.leaf_wgrad1x1: deferred, leaves of one shape in one grouped launch)
    def post(g, db):
        return {name + '.weight': g.view(Cout, Cin, 1, 1), name + '.bias': db} if has_b else {name + '.weight': g.view(Cout, Cin, 1, 1)}
    L.leaf_wgrad1x1((x, dout), (x, dout, Cout, Cin, False), post, G, want_db=has_b)
    wp, mp, *_ = K.pack_weights(w, PACK_DGRAD_S1)
    return K.conv_forward(dout, wp, mp, Cin, 1)


def _img_conv(x, Wt, Cout, out=None, bias=None, res=None):
    """1x1 conv with per-image weights Wt [N, Kp, Mp] (fp32 packed layout emitted by tdr_mdta_*): on the split-bf16
    kernel after one batched re-pack, or directly on the exact fp32 kernel (kernels.MATH)."""
    Kp, Mp = Wt.shape[-2], Wt.shape[-1]
    if K.MATH != 'f32':
        pw, per_b = K.pack_f32packed_to_bx3(Wt)
        return K.conv_forward(x, pw, Mp, Cout, 1, wp_ns=per_b, out=out, bias=bias, res=res)
    return K.conv_forward(x, Wt, Mp, Cout, 1, wp_ns=Kp * Mp, out=out, bias=bias, res=res)


def attn_tail_fwd(v, AT, P, heads, res, keep=True):
    """project_out(attn v) + res, the end of MDTA / TKSA.  v [N,C,H,W] (a channel slice of qkv), AT [N,Cp,Cp] -> (y, o); o = attn v is
    what project_out's weight gradient reads.  keep=False with INFER_FOLD: y = (Wo attn) v + bias + res in one convolution on the folded
    per-image weights, o never formed -> (y, None).  In every kernels.MATH but 'f32' the per-image weights run on the 3-way bf16 split
    (fp32 exponent range), so Wo attn -- which has Wo's range, not attn's [0, 1] -- sits in the operand window of each mode."""
    Cc = v.shape[1]
    if not keep and INFER_FOLD:
        return _img_conv(v, K.attn_fold_proj(AT, P['attn.project_out.weight'], heads), Cc, bias=P.get('attn.project_out.bias'), res=res), None
    o = _img_conv(v, AT, Cc)                                                     # attn v
    return _pw_fwd(o, P, 'attn.project_out', res=res), (o if keep else None)


# ---------------------------------------------------------------------------
# TransformerBlock (:318-331) = x + MDTA(LN(x)); + GDFN(LN(.))
# ---------------------------------------------------------------------------
def tblock_fwd(x, P, heads, ln_type, keep=True):
    """keep=False: a forward pass no backward follows -> (out, None); each intermediate goes once its last consumer is enqueued (live
    at the widest point, in planes of the block's C channels: x, y, t2 [5.32] and g [2.66]), and the attention tail is attn_tail_fwd's"""
    N, Cc, H, W = x.shape
    xn, mu1, rs1 = _ln_fwd(x, P, 'norm1.', ln_type)
    # ---- MDTA (:246-277)
    t = _pw_fwd(xn, P, 'attn.qkv')                                               # [N,3C,H,W]
    if not keep:
        xn = mu1 = rs1 = None
    qkv = K.dwconv_fwd(t, P['attn.qkv_dwconv.weight'], P.get('attn.qkv_dwconv.bias'))
    if not keep:
        t = None
    ss = K.row_sumsq(qkv, 2 * Cc)                                                # |q_i|^2, |k_j|^2
    Gm = K.conv_wgrad(qkv[:, Cc:2 * Cc], qkv[:, :Cc], Cc, Cc, 1, per_image=True, fp16_range=True).view(N, Cc, Cc)   # q k^T
    A, AT = K.mdta_softmax(Gm, ss, P['attn.temperature'], heads)
    y, o = attn_tail_fwd(qkv[:, 2 * Cc:], AT, P, heads, x, keep)
    if not keep:
        qkv = ss = Gm = A = AT = None
    # ---- GDFN (:223-241)
    yn, mu2, rs2 = _ln_fwd(y, P, 'norm2.', ln_type)
    t2 = _pw_fwd(yn, P, 'ffn.project_in')                                        # [N,2h,H,W]
    if not keep:
        yn = mu2 = rs2 = None
    g = K.dwgelu_fwd(t2, P['ffn.dwconv.weight'], P.get('ffn.dwconv.bias'))
    if not keep:
        t2 = None
    out = _pw_fwd(g, P, 'ffn.project_out', res=y)
    if not keep:
        return out, None
    return out, (x, xn, mu1, rs1, t, qkv, ss, Gm, A, o, y, yn, mu2, rs2, t2, g)


def tblock_bwd(dout, P, heads, ln_type, saved):
    x, xn, mu1, rs1, t, qkv, ss, Gm, A, o, y, yn, mu2, rs2, t2, g = saved
    N, Cc, H, W = x.shape
    G = {}
    # ---- GDFN
    dg = _pw_bwd(dout, g, P, 'ffn.project_out', G)
    b = P.get('ffn.dwconv.bias')
    dt2, G['ffn.dwconv.weight'], db = K.dwgelu_bwd(dg, t2, P['ffn.dwconv.weight'], b)
    if b is not None:
        G['ffn.dwconv.bias'] = db
    dyn = _pw_bwd(dt2, yn, P, 'ffn.project_in', G)
    dy = _ln_bwd(dyn, y, mu2, rs2, P, 'norm2.', ln_type, G, add=dout)
    # ---- MDTA
    do = _pw_bwd(dy, o, P, 'attn.project_out', G)
    dA = K.conv_wgrad(qkv[:, 2 * Cc:], do, Cc, Cc, 1, per_image=True).view(N, Cc, Cc)      # dA_ij = do_i . v_j
    Wm, G['attn.temperature'] = K.mdta_bwd(Gm, ss, P['attn.temperature'], A, dA, heads)
    dqkv = torch.empty_like(qkv)
    _img_conv(do, A, Cc, out=dqkv[:, 2 * Cc:])                                             # dv = attn^T do
    _img_conv(qkv[:, :2 * Cc], Wm, 2 * Cc, out=dqkv[:, :2 * Cc])                           # d[q;k] = W [q;k]
    has_b = 'attn.qkv_dwconv.bias' in P
    dt, G['attn.qkv_dwconv.weight'], db = K.dwconv_bwd(dqkv, t, P['attn.qkv_dwconv.weight'], want_db=has_b)
    if has_b:
        G['attn.qkv_dwconv.bias'] = db
    dxn = _pw_bwd(dt, xn, P, 'attn.qkv', G)
    dx = _ln_bwd(dxn, x, mu1, rs1, P, 'norm1.', ln_type, G, add=dy)
    L.maybe_join()
    return dx, G


# TransformerResFusionBlock (:334-353): block(x) * alpha + x, around the network's TransformerBlock pair (tblock_fwd / tblock_bwd
# here, drsformer_engine's TKSA / MSFN blocks there)
def fblock_fwd(x, P, heads, ln_type, tblock=tblock_fwd, keep=True):
    z, sv = tblock(x, P, heads, ln_type, **_kw(keep))
    return K.axpby_dev(z, P['alpha'], x), ((sv, z) if keep else None)


def fblock_bwd(dout, P, heads, ln_type, saved, tblock=tblock_bwd):
    sv, z = saved
    dalpha = K.dot(dout, z)
    dz = K.axpby_dev(dout, P['alpha'])
    with L.deferred_join():
        dx, G = tblock(dz, P, heads, ln_type, sv)
    G['alpha'] = dalpha
    dx = K.add_(dx, dout)
    L.maybe_join()
    return dx, G


def seq_fwd(x, P, pre, n, heads, ln_type, tblock=tblock_fwd, fusion=False, keep=True):
    saved, kw = [], _kw(keep)
    for i in range(n):
        Pi = E._sub(P, f'{pre}{i}.')
        x, sv = fblock_fwd(x, Pi, heads, ln_type, tblock, **kw) if fusion else tblock(x, Pi, heads, ln_type, **kw)
        saved.append(sv)
    return x, (saved if keep else None)


def seq_bwd(d, P, pre, n, heads, ln_type, saved, G, tblock=tblock_bwd, fusion=False):
    for i in reversed(range(n)):
        L.set_prefix(f'{pre}{i}.')
        Pi = E._sub(P, f'{pre}{i}.')
        d, g = fblock_bwd(d, Pi, heads, ln_type, saved[i], tblock) if fusion else tblock(d, Pi, heads, ln_type, saved[i])
        E._put(G, f'{pre}{i}.', g)
    L.set_prefix('')                   # (top-level leaves -- reduce_chan_level*, skip_conv -- carry full names)
    return d


def refine_fwd(x, P, cfg, keep=True):
    """the `refinement.` TransformerBlocks after decoder_level1 (Restormer, PromptIR): a `tail` stage of walk_fwd"""
    return seq_fwd(x, P, 'refinement.', cfg['num_refinement_blocks'], cfg['heads'][0], cfg['LayerNorm_type'], keep=keep)


def refine_bwd(d, P, cfg, saved, G):
    return seq_bwd(d, P, 'refinement.', cfg['num_refinement_blocks'], cfg['heads'][0], cfg['LayerNorm_type'], saved, G)


# ---------------------------------------------------------------------------
# Downsample / Upsample (:370-391): 3x3 conv (no bias) + PixelUnshuffle(2) / PixelShuffle(2)
# ---------------------------------------------------------------------------
def down_fwd(x, w):
    return K.pixel_unshuffle2(E.conv_fwd(x, w, None, 1, 1))


def down_bwd(dout, x, w):
    dx, dw, _ = E.conv_bwd(K.pixel_shuffle2(dout), x, w, 1, 1, bias=False)
    return dx, dw


def up_fwd(x, w):
    wp, mp, *_ = K.pack_weights(w, PACK_FWD)
    return K.conv_forward(x, wp, mp, w.shape[0], 3, pad=1, epi=EPI_PSHUF)


def up_bwd(dout, x, w):
    dx, dw, _ = E.conv_bwd(K.pixel_unshuffle2(dout), x, w, 1, 1, bias=False)
    return dx, dw


def _conv_bwd(dout, x, P, name, G, need_dx=True):
    """3x3 conv `name` (patch_embed.proj, output) on E.conv_bwd's immediate path: stores dW, and db if the conv has a bias"""
    has_b = name + '.bias' in P
    dx, G[name + '.weight'], db = E.conv_bwd(dout, x, P[name + '.weight'], 1, 1, need_dx=need_dx, bias=has_b)
    if has_b:
        G[name + '.bias'] = db
    return dx


# ---------------------------------------------------------------------------
# the 4-level U-Net of the whole family (RestormerRefFusion.forward :751-963, Restormer.forward :464-501, PromptIR, DRSformer):
# one forward walk, one backward walk; the networks differ only by the arguments their net_fwd / net_bwd pass
# ---------------------------------------------------------------------------
_FUS = ['masa_blk_enc_level1.', 'masa_blk_enc_level2.', 'masa_blk_enc_level3.', 'masa_blk_enc_level4.']
_ENC = ['encoder_level1.', 'encoder_level2.', 'encoder_level3.', 'latent.']
_DOWN = ['down1_2.body.0.weight', 'down2_3.body.0.weight', 'down3_4.body.0.weight']
_UP = ['up2_1.body.0.weight', 'up3_2.body.0.weight', 'up4_3.body.0.weight']        # _UP[l]: into decoder level l + 1


def walk_fwd(P, cfg, inp, ref, size_msg, tblock=tblock_fwd, fuse=range(4), head=None, pre_up=None, tail=None, dual_pixel=False,
             keep=True):
    """inp [N,C,H,W] -> (out, saved).
    ref [N,C,Hr,Wr]: guided -- MASA pyramids and match (engine.pyramids_fwd / masa_fwd), zero padding to the MASA block grid
    (reference defect R1: the pyramid is [L1..L4], padder_size 8), a fusion stage (fusion blocks on cat[x, warp_l], then the
    first half of the channels) at each level in `fuse`.  ref None: un-guided -- no reference branch and no padding: H, W must be
    multiples of 8 (the reference's PixelUnshuffle raises otherwise), else ValueError(size_msg.format(H, W)).
    What the caller passes in:
      tblock               TransformerBlock forward (x, P, heads, ln_type); the fusion blocks wrap it
      head(x, P, cfg)      stage after the patch embedding -> (x, saved)
      pre_up(x, P, cfg, l) stage before the Upsample into decoder level l (l = 3, 2, 1) -> (x, saved)
      tail(x, P, cfg)      stage after decoder_level1 -> (x, saved)
      dual_pixel           output(x + skip_conv(inp_enc_level1)) without `+ inp` (Restormer's dual-pixel task, :955-959)
    saved = (N, (H0, W0, Hp, Wp), geo, pyr, None, None, sv_masa, S) -- the prefix of engine.net_fwd's; S holds the rest by name.
    keep=False: a forward pass no backward follows (inference, validation) -> (out, None); tblock and the stages are called with
    keep=False and return (x, None).  Live at any moment: the warped reference features of the levels still to come, the encoder outputs
    of the levels passed (each until its decoder level has concatenated it), the padded input (the output conv's residual) and one
    block's working set -- the pyramids go behind the transfer kernels, a concat buffer when the level's first fusion block has read it,
    `inp_enc_level1` at once unless dual_pixel."""
    N = inp.shape[0]
    kw = _kw(keep)
    if ref is not None:
        pyr, sizes = E.pyramids_fwd(P, cfg, inp, ref, PADDER_LOG2, 4, **kw)
        warp, sv_masa = E.masa_fwd(pyr.lq_deep, pyr.ref_feats, N, pyr.geo, **kw)
        if not keep:
            pyr.lq_deep = pyr.ref_feats = None
            warp = [w if l in fuse else None for l, w in enumerate(warp)]
    else:
        H, W = inp.shape[2:]
        if H % 8 or W % 8:
            raise ValueError(size_msg.format(H, W))
        pyr, sizes, sv_masa, fuse = types.SimpleNamespace(inp_p=inp.contiguous(), geo=None), (H, W, H, W), None, ()
    hd, ln, nb, nfz = cfg['heads'], cfg['LayerNorm_type'], cfg['num_blocks'], cfg.get('reffusion_n_blocks')
    S = types.SimpleNamespace(levels=[], dec=[None] * 3) if keep else None      # what walk_bwd reads, by name
    enc, x_l1, sv_h, sv_t = [], None, None, None
    x = E.conv_fwd(pyr.inp_p, P['patch_embed.proj.weight'], P.get('patch_embed.proj.bias'), 1, 1)
    if head:
        x, sv_h = head(x, P, cfg, **kw)
    for l in range(4):
        sv_f = None
        if l in fuse:
            arg, c = [K.concat2(x, warp[l])], x.shape[1]
            if not keep:
                x = warp[l] = None
            f, sv_f = seq_fwd(E._take(arg, 0), P, _FUS[l], nfz[l], hd[l], ln, tblock, fusion=True, **kw)
            x = K.slice_channels(f, 0, c)                  # `[:, :embed_dim // 2]` (:892,903,914,925)
            f = None
        if l == 0 and (keep or dual_pixel):
            x_l1 = x                                       # `inp_enc_level1`: what skip_conv reads when dual_pixel
        arg = [x]
        if not keep:
            x = None
        e, sv_e = seq_fwd(E._take(arg, 0), P, _ENC[l], nb[l], hd[l], ln, tblock, **kw)
        enc.append(e if keep or l < 3 else None)
        if keep:
            S.levels.append((sv_f, sv_e))
        if l < 3:
            x = down_fwd(e, P[_DOWN[l]])
    x, e = e, None                                         # the latent
    for l in (2, 1, 0):                                    # decoder level l + 1 on cat[Upsample(x), encoder level l + 1]
        sv_p = None
        if pre_up:
            x, sv_p = pre_up(x, P, cfg, l + 1, **kw)
        cat = K.concat2(up_fwd(x, P[_UP[l]]), enc[l])
        arg = [_pw_fwd(cat, P, f'reduce_chan_level{l + 1}') if l else cat]
        if not keep:
            x = cat = enc[l] = None
        y, sv_d = seq_fwd(E._take(arg, 0), P, f'decoder_level{l + 1}.', nb[l], hd[l], ln, tblock, **kw)
        if keep:
            S.dec[l] = (sv_p, x, cat, sv_d)
        x = y
    y = None
    if tail:
        x, sv_t = tail(x, P, cfg, **kw)
    if dual_pixel:
        x = _pw_fwd(x_l1, P, 'skip_conv', res=x)
        if not keep:
            x_l1 = None
    out_p = E.conv_fwd(x, P['output.weight'], P.get('output.bias'), 1, 1, res=None if dual_pixel else pyr.inp_p)
    H0, W0, Hp, Wp = sizes
    out = out_p if (Hp, Wp) == (H0, W0) else K.pad_crop(out_p, H0, W0)
    if not keep:
        return out, None
    S.head, S.tail, S.enc, S.x_l1, S.y = sv_h, sv_t, enc, x_l1, x
    return out, (N, sizes, pyr.geo, pyr, None, None, sv_masa, S)


def walk_bwd(dout, P, cfg, saved, G=None, tblock=tblock_bwd, head=None, pre_up=None, tail=None, dual_pixel=False, late=True):
    """-> G, the parameter gradients of walk_fwd (the input image is data).  The stages are the backward of the ones passed to
    walk_fwd: head(d, P, cfg, saved, G), pre_up(d, P, cfg, l, saved, G), tail(d, P, cfg, saved, G) -> gradient of the stage input.
    late: leaf weight gradients queued (engine.late_leaves) and run next to the MASA backward at the end (leaves.run_late_leaves)."""
    G = {} if G is None else G
    with L.deferred_join(), (E.late_leaves(G) if late else contextlib.nullcontext()):
        N, (H0, W0, Hp, Wp), _, pyr, _, _, sv_masa, S = saved
        hd, ln, nb, nfz = cfg['heads'], cfg['LayerNorm_type'], cfg['num_blocks'], cfg.get('reffusion_n_blocks')
        dout = dout.contiguous()
        if (Hp, Wp) != (H0, W0):
            dout = K.pad_crop(dout, Hp, Wp)
        d = _conv_bwd(dout, S.y, P, 'output', G)
        dskip_l1 = _pw_bwd(d, S.x_l1, P, 'skip_conv', G) if dual_pixel else None
        if tail:
            d = tail(d, P, cfg, S.tail, G)
        dskip = []
        for l in range(3):
            sv_p, xu, cat, sv_d = S.dec[l]
            d = seq_bwd(d, P, f'decoder_level{l + 1}.', nb[l], hd[l], ln, sv_d, G, tblock)
            if l:
                d = _pw_bwd(d, cat, P, f'reduce_chan_level{l + 1}', G)
            cu = d.shape[1] - S.enc[l].shape[1]            # d = grad of cat[Upsample(xu), encoder output]
            dskip.append(d[:, cu:])
            d, G[_UP[l]] = up_bwd(K.slice_channels(d, 0, cu), xu, P[_UP[l]])
            if pre_up:
                d = pre_up(d, P, cfg, l + 1, sv_p, G)
        dwarp = [None] * 4
        for l in reversed(range(4)):
            sv_f, sv_e = S.levels[l]
            d = seq_bwd(d, P, _ENC[l], nb[l], hd[l], ln, sv_e, G, tblock)
            if l == 0 and dskip_l1 is not None:
                d = K.add_(d, dskip_l1)
            c, H, W = d.shape[1:]
            if sv_f is not None:
                df = torch.zeros(N, 2 * c, H, W, dtype=torch.float32, device=d.device)
                K.copy_rows(d, c * H * W, df, 2 * c * H * W, N, c * H * W)
                dcat = seq_bwd(df, P, _FUS[l], nfz[l], hd[l], ln, sv_f, G, tblock, fusion=True)
                dwarp[l] = dcat[:, c:]
                d = K.slice_channels(dcat, 0, c)
            elif sv_masa is not None:                      # a guided level without fusion (DRSformer's R6): its warp gets no gradient
                dwarp[l] = torch.zeros(N, c, H, W, dtype=torch.float32, device=d.device)
            if l > 0:
                d, G[_DOWN[l - 1]] = down_bwd(d, S.enc[l - 1], P[_DOWN[l - 1]])
                d = K.add_(d, dskip[l - 1])
        if head:
            d = head(d, P, cfg, S.head, G)
        _conv_bwd(d, pyr.inp_p, P, 'patch_embed.proj', G, need_dx=False)
        if late:
            L.run_late_leaves(G, lambda: E.pyramids_bwd(dwarp, pyr, P, cfg, sv_masa, G) if sv_masa is not None else None)
    return G


# ---------------------------------------------------------------------------
# whole network: RestormerRefFusion (ref given) and the un-guided Restormer (ref None)
# ---------------------------------------------------------------------------
def net_fwd(P, cfg, inp, ref, keep=True):
    """inp, ref [N,3,H,W] -> (out [N,3,H,W], saved).  cfg: constructor kwargs of RestormerRefFusion / Restormer.
    keep=False: (out, None), nothing kept for a backward pass (walk_fwd)"""
    return walk_fwd(P, cfg, inp, ref, 'Restormer: H, W must be multiples of 8 (three PixelUnshuffle(2) stages, :370-378); got {}x{}',
                    tail=refine_fwd, dual_pixel=cfg.get('dual_pixel_task'), keep=keep)


def net_bwd(dout, P, cfg, saved, G=None):
    # the un-guided Restormer runs its leaves at once: grouped 1x1 weight gradients are not bit-identical to ungrouped ones
    return walk_bwd(dout, P, cfg, saved, G, tail=refine_bwd, dual_pixel=cfg.get('dual_pixel_task'), late=saved[6] is not None)
