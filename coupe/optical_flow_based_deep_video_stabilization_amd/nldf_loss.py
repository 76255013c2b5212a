"""NLDF's objective over the HIP calls of csrc/nldf_loss_ops.hip (C ABI in include/vstab.h): what `NLDF.Model.im_gradient`, `Loss_IoU`,
`Loss_Contour`, `L2`, `build_loss`, `NLDF.saliency_loss` and `vgg16.Vgg16.L2` run on.  float32 CUDA tensors only; there is no CPU
path.  Every value and gradient is summed without atomics in a fixed order: two runs give the same bits.

One departure from TensorFlow's gradient: where a channel's Sobel magnitude is exactly 0 its derivative is taken as 0 (TensorFlow's
sqrt gradient gives inf * 0 = NaN there, and a saturated softmax produces such pixels)."""
from __future__ import annotations

from collections import namedtuple

import torch
from torch.autograd.function import once_differentiable

from . import runtime
from ._autograd import wants_grad as _wants_grad
from .runtime import ptr as _ptr

REDUCE_IOU, REDUCE_CONTOUR, REDUCE_L2 = 0, 1, 2          # VSTAB_NLDF_REDUCE_*

SaliencyLoss = namedtuple("SaliencyLoss", "Loss_Mean C_IoU_LOSS CE accuracy Prob_Grad label_Grad")


# ---- im_gradient
def sobel_magnitude(im):
    B, H, W, C = im.shape
    out = torch.empty_like(im)
    runtime.call(im.device, "vstab_sobel_magnitude", im.data_ptr(), B, H, W, C, out.data_ptr())
    return out


def sobel_magnitude_backward(im, dout):
    """The adjoint of im_gradient at `im` applied to dout (both [B,H,W,C]): gathered, no atomics; what the autograd function calls."""
    im = runtime.f32_cuda(im, "im", 4, layout="[B,H,W,C]")
    dout = runtime.f32_cuda(dout, "dout", 4, layout="[B,H,W,C]")
    if dout.shape != im.shape or dout.device != im.device:
        raise ValueError("dout must have im's shape and device")
    B, H, W, C = im.shape
    dx = torch.empty_like(im)
    runtime.call(im.device, "vstab_sobel_magnitude_backward", im.data_ptr(), dout.data_ptr(), B, H, W, C, dx.data_ptr())
    return dx


class _SobelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, im):
        ctx.save_for_backward(im)
        return sobel_magnitude(im)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return sobel_magnitude_backward(ctx.saved_tensors[0], dout.contiguous())


def im_gradient(im):
    im = runtime.f32_cuda(im, "im", 4, layout="[B,H,W,C]")
    if not 1 <= im.shape[3] <= 4:
        raise ValueError(f"im has {im.shape[3]} channels: 1..4 are built")
    return _SobelFn.apply(im) if _wants_grad(im) else sobel_magnitude(im)


# ---- the scalar reductions
def reduce_call(mode, a, b, wd, want_grad):
    """(value, d value / d a or None) of VSTAB_NLDF_REDUCE_* `mode` over the flattened a (and b)."""
    n = a.numel()
    ws = runtime.workspace(a.device, "vstab_nldf_reduce_workspace_bytes", n, refused=f"need 1 .. 2^31 - 1 elements, got {n}")
    value = torch.empty((), dtype=torch.float32, device=a.device)
    grad = torch.empty_like(a) if want_grad else None
    runtime.call(a.device, "vstab_nldf_reduce", mode, a.data_ptr(), _ptr(b), n, float(wd), value.data_ptr(), _ptr(grad), ws.data_ptr(), ws.numel())
    return value, grad


class _ReduceFn(torch.autograd.Function):
    """The gradient comes out of the forward's call (one more launch) and is scaled by the upstream scalar."""

    @staticmethod
    def forward(ctx, mode, wd, a, b):
        value, grad = reduce_call(mode, a, b, wd, True)
        ctx.save_for_backward(grad)
        return value

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return None, None, ctx.saved_tensors[0] * dout, None


def _reduce(mode, a, b, wd, names):
    a = runtime.f32_cuda(a, names[0])
    if b is not None:
        b = runtime.f32_cuda(b, names[1])
        if b.requires_grad:
            raise ValueError(f"{names[1]} requires grad: only {names[0]} is differentiated (detach {names[1]})")
        if b.numel() != a.numel() or b.device != a.device:
            raise ValueError(f"{names[0]} and {names[1]} must have the same number of elements and device")
    if _wants_grad(a):
        return _ReduceFn.apply(mode, wd, a, b)
    return reduce_call(mode, a, b, wd, False)[0]


def loss_iou(pred, gt):
    return _reduce(REDUCE_IOU, pred, gt, 0.0, ("pred", "gt"))


def loss_contour(pred, gt):
    return _reduce(REDUCE_CONTOUR, pred, gt, 0.0, ("pred", "gt"))


def l2(tensor, wd):
    return _reduce(REDUCE_L2, tensor, None, wd, ("tensor",))


# ---- the fused loss
def saliency_loss_call(score, label, contour_th=1.5, want_maps=True, want_dscore=False, dscale=1.0):
    """One vstab_nldf_loss call on score, label [B,H,W,2]: (scalars [4] = Loss_Mean, C_IoU_LOSS, CE, accuracy; Prob_Grad, label_Grad
    [B,H,W,1] or None; dscore = dscale * d Loss_Mean / d score or None).  The raw entry: no autograd."""
    score = runtime.f32_cuda(score, "score", 4, 2, "[B,H,W,2]")
    label = runtime.f32_cuda(label, "label", 4, 2, "[B,H,W,2]")
    if label.shape != score.shape or label.device != score.device:
        raise ValueError("score and label must have the same shape and device")
    B, H, W, _ = score.shape
    dev = score.device
    ws = runtime.workspace(dev, "vstab_nldf_loss_workspace_bytes", B, H, W,
                           refused=f"saliency_loss: need B, H, W >= 1 and fewer than 2^31 elements, got {B}x{H}x{W}x2")
    scalars = torch.empty(4, dtype=torch.float32, device=dev)
    pg = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev) if want_maps else None
    lg = torch.empty((B, H, W, 1), dtype=torch.float32, device=dev) if want_maps else None
    dscore = torch.empty_like(score) if want_dscore else None
    runtime.call(dev, "vstab_nldf_loss", score.data_ptr(), label.data_ptr(), B, H, W, float(contour_th), scalars.data_ptr(), _ptr(pg), _ptr(lg),
                 _ptr(dscore), float(dscale), ws.data_ptr(), ws.numel())
    return scalars, pg, lg, dscore


class _SaliencyLossFn(torch.autograd.Function):
    """Loss_Mean with d Loss_Mean / d score from the same fused call; the other outputs carry no gradient."""

    @staticmethod
    def forward(ctx, score, label, contour_th):
        scalars, pg, lg, dscore = saliency_loss_call(score, label, contour_th, True, True)
        ctx.save_for_backward(dscore)
        rest = (scalars[1], scalars[2], scalars[3], pg, lg)
        ctx.mark_non_differentiable(*rest)
        return (scalars[0],) + rest

    @staticmethod
    @once_differentiable
    def backward(ctx, dloss, *unused):
        return ctx.saved_tensors[0] * dloss, None, None


def saliency_loss(score, label, contour_th=1.5):
    """NLDF.py:79-100 on score, label [B,H,W,2] float32 CUDA (label: per pixel a distribution over the two classes):
    SaliencyLoss(Loss_Mean, C_IoU_LOSS, CE, accuracy, Prob_Grad, label_Grad).  Loss_Mean = C_IoU_LOSS + CE is differentiable with respect
    to score, through the fused HIP backward; C_IoU_LOSS, CE and accuracy (0-dim) and the two [B,H,W,1] maps carry no gradient, and a
    label that requires grad raises."""
    if torch.is_tensor(label) and label.requires_grad:
        raise ValueError("label requires grad: only score is differentiated (detach label)")
    if torch.is_tensor(score) and _wants_grad(score):
        score = runtime.f32_cuda(score, "score", 4, 2, "[B,H,W,2]")
        return SaliencyLoss(*_SaliencyLossFn.apply(score, label, float(contour_th)))
    scalars, pg, lg, _ = saliency_loss_call(score, label, contour_th)
    return SaliencyLoss(scalars[0], scalars[1], scalars[2], scalars[3], pg, lg)
