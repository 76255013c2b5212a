"""Drop-ins for the warp ops the reference defines inside its main scripts:
`tf_warp` (main:70-130), `get_pixel_value` (main:44-68) and the flow glue of
`evaluate_originalSize` (main:497-498) and `evaluate` (main:806).
("main" = main_flownetS_pyramid_noprevloss_dataloader.py.)  HIP kernels only.

Differentiable (torch.autograd, HIP backward kernels behind `sampler_grad.*_backward`): `tf_warp` with respect to the image and the flow,
`get_pixel_value` with respect to the image, `resize_images` / `resize_images_slice3` with respect to their input,
`flow_to_output_res` with respect to predict_flow2, `flow_glue_warp` with respect to predict_flow2 and the frame.  The gradients are
what TensorFlow's autodiff yields: tf_warp's corner indices come from integer casts and carry no gradient, the flow enters through the
four weights of the clipped corners only.  Image gradients of the two gathers are summed by float atomics (last bits may differ
between runs); the flow gradients and the resize adjoints are bit-reproducible.  The autograd path is taken only when gradients are
enabled and an input requires grad; otherwise the calls are the forward launches alone and the results carry no `grad_fn`."""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _autograd, runtime, sampler_grad
from ._autograd import wants_grad as _wants_grad
from .runtime import f32_cuda as _f32_cuda


def _tf_warp_call(img, flow):
    B, H, W, Cc = img.shape
    out = torch.empty_like(img)
    runtime.call(img.device, "vstab_warp_flow", img.data_ptr(), flow.data_ptr(), out.data_ptr(), B, H, W, Cc)
    return out


def _tf_warp_backward(saved, dout, needs, statics):
    """d img and / or d flow, whichever is needed."""
    return sampler_grad.warp_flow_backward(*saved, dout, need_img=needs[0], need_flow=needs[1])


def tf_warp(img, flow, H, W):
    """img [B,H,W,C], flow [B,H,W,2] (channel 0 = x, 1 = y) -> warped [B,H,W,C].  Differentiable with respect to img and flow."""
    img = _f32_cuda(img, "img")
    flow = _f32_cuda(flow, "flow")
    B, h, w, Cc = img.shape
    if (h, w) != (H, W) or tuple(flow.shape) != (B, H, W, 2):
        raise ValueError(f"tf_warp: img {tuple(img.shape)} / flow {tuple(flow.shape)} do not match H={H}, W={W}")
    return _autograd.apply(_tf_warp_call, _tf_warp_backward, (img, flow))


def _get_pixel_value_call(img, x, y):
    B, Hi, Wi, Cc = img.shape
    _, H, W = x.shape
    out = torch.empty((B, H, W, Cc), dtype=torch.float32, device=img.device)
    runtime.call(img.device, "vstab_get_pixel_value", img.data_ptr(), x.data_ptr(), y.data_ptr(), out.data_ptr(), B, H, W, Cc, Hi, Wi)
    return out


class _GetPixelValueFn(torch.autograd.Function):
    """get_pixel_value with its HIP backward (sampler_grad.get_pixel_value_backward): the scatter-add into d img."""

    @staticmethod
    def forward(ctx, img, x, y):
        ctx.save_for_backward(x, y)
        ctx.img_hw = tuple(img.shape[1:3])
        return _get_pixel_value_call(img, x, y)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        x, y = ctx.saved_tensors
        return sampler_grad.get_pixel_value_backward(dout, x, y, ctx.img_hw), None, None


def get_pixel_value(img, x, y):
    """img [B,Hi,Wi,C]; x, y int32 [B,H,W] -> img[b, y, x, :] as [B,H,W,C].  Differentiable with respect to img."""
    img = _f32_cuda(img, "img")
    if x.shape != y.shape or x.dim() != 3:
        raise ValueError("x and y must both be [B,H,W]")
    x = x.to(device=img.device, dtype=torch.int32).contiguous()
    y = y.to(device=img.device, dtype=torch.int32).contiguous()
    if _wants_grad(img):
        return _GetPixelValueFn.apply(img, x, y)
    return _get_pixel_value_call(img, x, y)


def _resize_call(x, oh, ow):
    B, h, w, Cc = x.shape
    out = torch.empty((B, oh, ow, Cc), dtype=torch.float32, device=x.device)
    runtime.call(x.device, "vstab_resize_bilinear", x.data_ptr(), B, h, w, Cc, out.data_ptr(), oh, ow)
    return out


class _ResizeFn(torch.autograd.Function):
    """resize_images with the adjoint of the legacy bilinear resize (sampler_grad.resize_bilinear_backward; atomic-free)."""

    @staticmethod
    def forward(ctx, x, oh, ow):
        ctx.in_hw = tuple(x.shape[1:3])
        return _resize_call(x, oh, ow)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return sampler_grad.resize_bilinear_backward(dout, ctx.in_hw), None, None


def resize_images(x, size):
    """tf.image.resize_images(x, size): legacy bilinear, align_corners=False (main:806).  Differentiable with respect to x."""
    x = _f32_cuda(x, "x")
    oh, ow = int(size[0]), int(size[1])
    if _wants_grad(x):
        return _ResizeFn.apply(x, oh, ow)
    return _resize_call(x, oh, ow)


def _resize_slice3_call(x, c_off, oh, ow):
    B, h, w, Cs = x.shape
    out = torch.empty((B, oh, ow, 3), dtype=torch.float32, device=x.device)
    runtime.call(x.device, "vstab_resize_bilinear_slice3", x.data_ptr(), B, h, w, Cs, int(c_off), out.data_ptr(), oh, ow)
    return out


class _ResizeSlice3Fn(torch.autograd.Function):
    """resize_images_slice3: the three channels' adjoint by sampler_grad.resize_bilinear_backward, placed into a zero tensor of x's shape."""

    @staticmethod
    def forward(ctx, x, c_off, oh, ow):
        ctx.in_shape, ctx.c_off = tuple(x.shape), c_off
        return _resize_slice3_call(x, c_off, oh, ow)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        dx = torch.zeros(ctx.in_shape, dtype=torch.float32, device=dout.device)
        dx[..., ctx.c_off:ctx.c_off + 3] = sampler_grad.resize_bilinear_backward(dout, ctx.in_shape[1:3])
        return dx, None, None, None


def resize_images_slice3(x, c_off, size):
    """resize_images(x[..., c_off:c_off+3], size) read in place from the Cs-channel tensor (main:806: the unstable frame is
    channels 24:27 of the input stack) -- no intermediate 3-channel copy; bit-identical to resize_images of that copy.
    Differentiable with respect to x (the other channels' gradient is zero)."""
    x = _f32_cuda(x, "x")
    B, h, w, Cs = x.shape
    oh, ow = int(size[0]), int(size[1])
    if (h, w) == (oh, ow):
        return x[..., c_off:c_off + 3].contiguous()
    if _wants_grad(x):
        return _ResizeSlice3Fn.apply(x, int(c_off), oh, ow)
    return _resize_slice3_call(x, c_off, oh, ow)


def _flow_to_output_res_call(f, net_h, net_w, out_h, out_w):
    B, h, w, two = f.shape
    out = torch.empty((B, out_h, out_w, 2), dtype=torch.float32, device=f.device)
    runtime.call(f.device, "vstab_flow_resize_scale", f.data_ptr(), B, h, w, out.data_ptr(), out_h, out_w, int(net_h), int(net_w))
    return out


class _FlowToOutputResFn(torch.autograd.Function):
    """flow_to_output_res with its adjoint (sampler_grad.flow_resize_scale_backward; atomic-free)."""

    @staticmethod
    def forward(ctx, f, net_h, net_w, out_h, out_w):
        ctx.in_hw, ctx.net = tuple(f.shape[1:3]), (net_h, net_w)
        return _flow_to_output_res_call(f, net_h, net_w, out_h, out_w)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        return sampler_grad.flow_resize_scale_backward(dout, ctx.in_hw, *ctx.net), None, None, None, None


def flow_to_output_res(predict_flow2, net_h, net_w, out_h, out_w):
    """main:497-498 with 384 -> net_h, 512 -> net_w:
    resize_images(pf2 * net_h / pf2.shape[1], [out_h, out_w]); x = x * out_w / net_w; y = y * out_h / net_h
    (each `*` and `/` its own fp32 operation, in the reference's order).  Differentiable with respect to predict_flow2."""
    f = _f32_cuda(predict_flow2, "predict_flow2")
    B, h, w, two = f.shape
    if two != 2:
        raise ValueError("flow must have 2 channels")
    args = (int(net_h), int(net_w), int(out_h), int(out_w))
    if _wants_grad(f):
        return _FlowToOutputResFn.apply(f, *args)
    return _flow_to_output_res_call(f, *args)


def _flow_glue_warp_call(f, img, net_h, net_w, want_outflow):
    B, h, w, two = f.shape
    _, oh, ow, Cc = img.shape
    outflow = torch.empty((B, oh, ow, 2), dtype=torch.float32, device=f.device) if want_outflow else None
    out = torch.empty_like(img)
    runtime.call(f.device, "vstab_flow_glue_warp", f.data_ptr(), B, h, w, img.data_ptr(), runtime.ptr(outflow), out.data_ptr(), oh, ow, Cc,
                 int(net_h), int(net_w))
    return outflow, out


class _FlowGlueWarpFn(torch.autograd.Function):
    """flow_glue_warp (one fused launch) with its backward: the warp backward at output resolution, plus any gradient arriving on
    outflow, through the glue's adjoint.  Without want_outflow the output-resolution flow is recomputed by flow_to_output_res, which
    is bit-identical to what the fused launch used."""

    @staticmethod
    def forward(ctx, f, img, net_h, net_w, want_outflow):
        outflow, warped = _flow_glue_warp_call(f, img, net_h, net_w, want_outflow)
        ctx.net, ctx.want_outflow = (net_h, net_w), want_outflow
        ctx.set_materialize_grads(False)
        if want_outflow:
            ctx.save_for_backward(f, img, outflow)
            return outflow, warped
        ctx.save_for_backward(f, img)
        return warped

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        g_outflow, d_warped = grads if ctx.want_outflow else (None, grads[0])
        f, img = ctx.saved_tensors[:2]
        need_f, need_img = ctx.needs_input_grad[:2]
        d_img, d_of = None, None
        if d_warped is not None:
            oh, ow = img.shape[1:3]
            outflow = ctx.saved_tensors[2] if ctx.want_outflow else _flow_to_output_res_call(f, *ctx.net, oh, ow)
            d_img, d_of = sampler_grad.warp_flow_backward(img, outflow, d_warped, need_img=need_img, need_flow=need_f)
        d_f = None
        if need_f:
            if g_outflow is not None:
                d_of = g_outflow if d_of is None else d_of + g_outflow
            if d_of is not None:
                d_f = sampler_grad.flow_resize_scale_backward(d_of, f.shape[1:3], *ctx.net)
        return d_f, d_img, None, None, None


def flow_glue_warp(predict_flow2, frame, net_h, net_w, want_outflow=True):
    """main:497-514 in one launch: (outflow, warped) = (flow_to_output_res(pf2, ...), tf_warp(frame, outflow, oh, ow)) for a
    3-channel frame [B,oh,ow,3]; bit-identical to the two calls.  With want_outflow=False the output-resolution flow is never
    written and None is returned in its place.  Differentiable with respect to predict_flow2 and frame."""
    f = _f32_cuda(predict_flow2, "predict_flow2")
    img = _f32_cuda(frame, "frame")
    B, h, w, two = f.shape
    if two != 2 or img.dim() != 4 or img.shape[0] != B:
        raise ValueError(f"flow_glue_warp: flow {tuple(f.shape)} / frame {tuple(img.shape)} do not match")
    if _wants_grad(f, img):
        r = _FlowGlueWarpFn.apply(f, img, int(net_h), int(net_w), bool(want_outflow))
        return r if want_outflow else (None, r)
    return _flow_glue_warp_call(f, img, net_h, net_w, want_outflow)
