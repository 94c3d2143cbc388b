"""Hand-written forward/backward of PromptIR-ref (models/archs/network_promptir_guided_arch.py of the reference) on the
HIP kernels -- SURVEY.md 8f, the first of the "next" guided architectures.

The file's LayerNorm / MDTA / GDFN / TransformerBlock / TransformerResFusionBlock / Downsample / Upsample classes
(:176-400) are the ones of Restormer-ref, and the network is restormer_engine's U-Net walk (same MASA front-end: 4-level
pyramid, padder_size 8, reference defect R1).  New here: PromptGenBlock (:417-441, csrc/tdr_prompt.hip) and the prompt
stage before each Upsample of the decoder (:1057-1092), passed to the walk.  Only the `decoder=True`, dim = nf = 48 network exists: with `decoder=False` the
reference itself raises in up4_3 (defect R4, oracle/promptir_ref_oracle.py), and the prompt widths are hard-wired.
`chnl_reduce1-3` / `reduce_noise_channel_1-3` are registered by the reference but never used: they never reach this
engine (no gradient, as in the reference where their .grad stays None).
"""
from . import engine as E
from . import kernels as K
from . import leaves as L
from . import restormer_engine as R

# ---------------------------------------------------------------------------
# PromptGenBlock (:417-441)
# ---------------------------------------------------------------------------
def prompt_fwd(x, P, pre, keep=True):
    """x [N,C,H,W] -> prompt [N,D,H,W].  The softmax-weighted sum over the L components and the bilinear resize are both
    linear and commute: the L*D parameter planes are resized once per call, not once per image.  keep=False: (prompt, None)"""
    N, C, H, W = x.shape
    comp = P[pre + 'prompt_param'][0]                                   # [L, D, S, S]
    L, D, S, _ = comp.shape
    emb = K.plane_mean(x)
    w = K.prompt_weights_fwd(emb, P[pre + 'linear_layer.weight'], P[pre + 'linear_layer.bias'])
    Pi = comp if (H, W) == (S, S) else K.resize_bilinear(comp.contiguous(), H, W)
    mix = K.prompt_mix_fwd(w, Pi.contiguous())
    out = E.conv_fwd(mix, P[pre + 'conv3x3.weight'], None, 1, 1)
    return out, ((x.shape, emb, w, Pi, mix) if keep else None)


def prompt_bwd(dout, P, pre, saved, G):
    """returns demb-broadcast information (demb [N,C], 1/HW): the caller adds it to the gradient of x."""
    (N, C, H, W), emb, w, Pi, mix = saved
    comp = P[pre + 'prompt_param']
    L, D, S = comp.shape[1], comp.shape[2], comp.shape[3]
    dmix, G[pre + 'conv3x3.weight'], _ = E.conv_bwd(dout, mix, P[pre + 'conv3x3.weight'], 1, 1, bias=False)
    dPi, dw = K.prompt_mix_bwd(w, Pi.contiguous(), dmix.contiguous())
    dcomp = dPi if (H, W) == (S, S) else K.resize_bilinear_bwd(dPi, S, S)
    G[pre + 'prompt_param'] = dcomp.view(1, L, D, S, S)
    G[pre + 'linear_layer.weight'], G[pre + 'linear_layer.bias'], demb = K.prompt_weights_bwd(
        emb, P[pre + 'linear_layer.weight'], w, dw)
    return demb, 1.0 / (H * W)


def _prompt_stage_fwd(x, P, cfg, k, keep=True):
    """the walk's stage before the Upsample into decoder level k (:1057-1084): cat([x, prompt_k(x)]) -> noise_level_k
    (TransformerBlock; all three use heads[2], :736, :747, :757) -> reduce_noise_level_k (1x1).  keep=False: (y, None)"""
    kw = R._kw(keep)
    pr, sv_p = prompt_fwd(x, P, f'prompt{k}.', **kw)
    cat = [K.concat2(x, pr)]
    if not keep:
        pr = None
    t, sv_t = R.tblock_fwd(E._take(cat, 0) if not keep else cat[0], E._sub(P, f'noise_level{k}.'), cfg['heads'][2], cfg['LayerNorm_type'], **kw)
    y = R._pw_fwd(t, P, f'reduce_noise_level{k}')
    return y, ((x.shape[1], sv_p, sv_t, t) if keep else None)


def _prompt_stage_bwd(d, P, cfg, k, saved, G):
    c, sv_p, sv_t, t = saved
    d = R._pw_bwd(d, t, P, f'reduce_noise_level{k}', G)
    L.set_prefix(f'noise_level{k}.')
    dcat, g = R.tblock_bwd(d, E._sub(P, f'noise_level{k}.'), cfg['heads'][2], cfg['LayerNorm_type'], sv_t)
    L.set_prefix('')
    E._put(G, f'noise_level{k}.', g)
    dx = K.slice_channels(dcat, 0, c)
    demb, inv = prompt_bwd(K.slice_channels(dcat, c, dcat.shape[1]), P, f'prompt{k}.', sv_p, G)
    return K.plane_add_(dx, demb, inv)


# ---------------------------------------------------------------------------
# whole network  PromptIRRefFusion.forward (:864-1092): restormer_engine's walk with the prompt stages and the refinement blocks
# ---------------------------------------------------------------------------
def net_fwd(P, cfg, inp, ref, keep=True):
    """keep=False: (out, None), nothing kept for a backward pass (restormer_engine.walk_fwd).  ref = None: the UN-GUIDED `PromptIR` of the same file (:443-590): no MASA pyramid, no fusion blocks, no padding (sizes must
    be multiples of 8).  Like the guided class it only exists as decoder=True, dim = 48 (with decoder=False its up4_3 receives
    the 384-channel latent on a 192-channel convolution and the reference raises: R4)."""
    if not cfg.get('decoder', True) or cfg['dim'] != 48 or (ref is not None and cfg['nf'] != 48):
        raise ValueError('PromptIR(-ref) exists only as decoder=True, dim = nf = 48 (the reference raises otherwise: defect R4)')
    return R.walk_fwd(P, cfg, inp, ref, 'PromptIR: H, W must be multiples of 8 (three PixelUnshuffle(2) stages); got {}x{}',
                      pre_up=_prompt_stage_fwd, tail=R.refine_fwd, keep=keep)


def net_bwd(dout, P, cfg, saved, G=None):
    return R.walk_bwd(dout, P, cfg, saved, G, pre_up=_prompt_stage_bwd, tail=R.refine_bwd)
