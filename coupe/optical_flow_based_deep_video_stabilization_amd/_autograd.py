"""The autograd plumbing every differentiable sampler shares (spatial_transformer.py, warp.py, warp_flow.py): one
`torch.autograd.Function` around "a forward launch that returns one tensor, and one `training.*_backward` call"."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable


def wants_grad(*tensors):
    return torch.is_grad_enabled() and any(t.requires_grad for t in tensors)


class SamplerFn(torch.autograd.Function):
    """out = call(*tensors, *statics).  The tensors are saved; `backward(saved, dout, needs, statics)` returns one gradient, or None,
    per tensor (needs: which of them require grad).  call, backward and statics get no gradient."""

    @staticmethod
    def forward(ctx, call, backward, statics, *tensors):
        ctx.save_for_backward(*tensors)
        ctx.backward_fn, ctx.statics = backward, statics
        return call(*tensors, *statics)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return (None, None, None, *ctx.backward_fn(ctx.saved_tensors, dout, ctx.needs_input_grad[3:], ctx.statics))


def apply(call, backward, tensors, statics=(), differentiable=True):
    """call(*tensors, *statics): through SamplerFn when gradients are enabled and a tensor requires grad, otherwise the launch alone.
    differentiable=False (the bicubic sampler without its opt-in) is always the launch alone."""
    if differentiable and wants_grad(*tensors):
        return SamplerFn.apply(call, backward, statics, *tensors)
    return call(*tensors, *statics)
