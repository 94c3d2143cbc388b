"""LayerNorm2d on the HIP kernels.  Mirrors models/archs/nafnet_arch_utils.py:264-300
of the reference (same class names, parameters `weight`/`bias`, eps 1e-6).  Also what every arch module shares: the device check
and the no-gradient forward route (infer_fwd)."""
import torch
import torch.nn as nn

from ... import kernels as K


def require_gpu(t, what):
    if not t.is_cuda:
        raise RuntimeError(f'{what}: the HIP path needs tensors on the MI355X; there is no CPU fallback '
                           '(the CPU oracle lives in oracle/ and is test infrastructure only).')


def infer_fwd(what, fwd, names, params, cfg, *images):
    """the forward pass when no gradient can be asked of its result -- grad mode is off (`torch.no_grad()`, as in torch; `.eval()`
    alone does not select it), or neither an image nor a parameter requires grad: the engine's whole-network forward `fwd` (net_fwd /
    unet_fwd of engine, restormer_engine, promptir_engine, drsformer_engine) with keep=False, outside autograd -> the output alone, or
    None when a gradient may be asked.  An image may be None (the un-guided networks of the Restormer family: ref=None).
    The weights are packed afresh from the parameters as they are now, outside any kernels.PackPlan: a validation pass between two
    optimiser steps must neither read a training step's cached packs nor record its own weights into that step's plan."""
    if torch.is_grad_enabled() and (any(t is not None and t.requires_grad for t in images) or any(p.requires_grad for p in params)):
        return None
    require_gpu(images[0], what)
    P = dict(zip(names, [p.detach() for p in params]))
    prev = K.set_pack_plan(None)
    try:
        with torch.no_grad():
            return fwd(P, cfg, *[t if t is None else t.detach() for t in images], keep=False)[0]
    finally:
        K.set_pack_plan(prev)


def infer_spec(net):
    """(fwd, names, params, cfg) of a network class routed through infer_fwd: the engine's whole-network forward in the shape
    `fwd(P, cfg, *images, keep=)` with the positional images of `net.forward`, the parameter names / tensors it reads (registration order,
    unused ones left out where the class does so) and the class's cfg.  Every such class answers with its `infer_spec()` method -- its own
    `forward` hands exactly this to infer_fwd, and inference.InferenceSession runs it under a pack plan of its own."""
    spec = getattr(net, 'infer_spec', None)
    if spec is None:
        raise TypeError(f'{type(net).__name__} has no infer_spec(): not a network routed through nafnet_arch_utils.infer_fwd')
    return spec()


def unguided(fwd):
    """the one-image form of a guided whole-network forward (Restormer / PromptIR / DRSformer without a reference: ref=None)"""
    def run(P, cfg, x, keep=True):
        return fwd(P, cfg, x, None, keep=keep)
    return run


class LayerNormFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        require_gpu(x, 'LayerNorm2d')
        x = x.contiguous()
        y, mu, rstd = K.layernorm2d_fwd(x, weight, bias, eps)
        ctx.save_for_backward(x, mu, rstd, weight)
        return y

    @staticmethod
    def backward(ctx, grad_output):
        x, mu, rstd, weight = ctx.saved_tensors
        gx, gw, gb = K.layernorm2d_bwd(grad_output.contiguous(), x, mu, rstd, weight)
        return gx, gw, gb, None


class LayerNorm2d(nn.Module):
    def __init__(self, channels, eps=1e-6):
        super().__init__()
        self.register_parameter('weight', nn.Parameter(torch.ones(channels)))
        self.register_parameter('bias', nn.Parameter(torch.zeros(channels)))
        self.eps = eps

    def forward(self, x):
        return LayerNormFunction.apply(x, self.weight, self.bias, self.eps)
