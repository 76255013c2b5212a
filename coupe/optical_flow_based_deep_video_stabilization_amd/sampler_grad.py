"""Backward of every sampler, one thin wrapper per library entry point: the spatial transformers, bilinear and bicubic
(`st_transform_backward`, `st_symmetry_transform_backward`, `st_elastic_transform_backward`, `st_bilinear_interp_backward`,
`st_bicubic_interp_backward`), the volume transformer (`st3d_*`), warp.py's homography warp and matrix exponential
(`homography_warp_backward`, `vec2mtrx_backward`) and warp_flow.py's tf_warp, get_pixel_value and resamplers.  What the autograd
functions of spatial_transformer.py, warp.py and warp_flow.py call; `training` re-exports every public name.

Everything runs in the HIP library (csrc/sampler_ops.hip, sampler3d_ops.hip, warp_flow_grad.hip, train_ops.hip); there is no CPU path."""
from __future__ import annotations

import math

import torch

from . import _lib, runtime
from .runtime import ptr as _ptr


def _st_backward_args(src, dout, out_size, d_src, need_src, rank=4):
    """The checks every sampler backward makes of its input (rank 4: img [B,H,W,C], out_size (oh, ow); rank 5: vol [B,D,H,W,C],
    out_size (od, oh, ow)), of dout and of a given gradient to add into -> (src, dout, src's shape + out_size, d_src, accumulate)."""
    name, layout = ("img", "[B,H,W,C]") if rank == 4 else ("vol", "[B,D,H,W,C]")
    src = runtime.f32_cuda(src, name, rank, layout=layout)
    out = tuple(int(out_size[i]) for i in range(rank - 2))
    counts = (src.shape[0], *out, src.shape[-1])
    if not torch.is_tensor(dout) or dout.device != src.device or dout.dtype != torch.float32 or dout.numel() != math.prod(counts):
        raise ValueError(f"dout must be a float32 tensor of {'*'.join(map(str, counts))} elements beside {name}")
    acc = d_src is not None
    if acc and (d_src.shape != src.shape or d_src.dtype != torch.float32 or d_src.device != src.device or not d_src.is_contiguous()):
        raise ValueError(f"d_{name} must be a contiguous float32 tensor of {name}'s shape beside it")
    if d_src is None and need_src:
        d_src = torch.empty_like(src)
    return src, dout.contiguous(), (*src.shape, *out), d_src, acc


def _backward_with_param_grad(entry, head, dout, out_size, d_src, acc, need_src, need_par, par_shape, ws_query, ws_args):
    """The call every sampler backward with a parameter gradient makes: entry(*head, dout, *out_size, d_src, accumulate, d_par,
    workspace, workspace_bytes, stream) -> (d_src or None, d_par or None).  entry and ws_query name the library's functions.  The
    parameter gradient [par_shape] and the workspace the library asks for (ws_query(*ws_args) bytes) exist only when need_par."""
    d_par, ws = None, None
    if need_par:
        d_par = torch.empty(par_shape, dtype=torch.float32, device=dout.device)
        ws = runtime.workspace(dout.device, ws_query, *ws_args)
    runtime.call(dout.device, entry, *head, dout.data_ptr(), *out_size, d_src.data_ptr() if need_src else None, 1 if acc else 0,
                 _ptr(d_par), _ptr(ws), ws.numel() if need_par else 0)
    return (d_src if need_src else None), d_par


def _st_interp(interp):
    if interp not in _lib.INTERP:
        raise ValueError("interp must be 'bilinear' or 'bicubic'")
    return _lib.INTERP[interp]


def _with_interp(entry, head, ip):
    """The bilinear sampler's entry point as it is; the bicubic one through `<entry>_interp_backward`, `interp` after the head."""
    return (entry, head) if ip == 0 else (entry.replace("_backward", "_interp_backward"), (*head, ip))


def st_transform_backward(img, theta, dout, out_size, need_img: bool = True, need_theta: bool = True, d_img=None, interp='bilinear'):
    """Gradients of AffineTransformer / ProjectiveTransformer.transform for the output gradient dout [B,oh,ow,C]: (d img [B,H,W,C] or
    None, d theta [B,6|8] or None).  A given d_img is added into (the `accumulate` convention), otherwise it is allocated and
    overwritten.  need_img / need_theta False skips that gradient's work.  d img is summed by float atomics (its last bits may differ
    between runs); d theta is bit-reproducible.  interp: the forward's sampler, 'bilinear' (the default: today's library call) or
    'bicubic' -- here and in the symmetric-pad and elastic backwards below."""
    ip = _st_interp(interp)
    need_img = need_img or d_img is not None
    img, dout, (B, H, W, C, oh, ow), d_img, acc = _st_backward_args(img, dout, out_size, d_img, need_img)
    theta = theta.contiguous()
    if not theta.is_cuda or theta.dtype != torch.float32 or theta.numel() not in (6 * B, 8 * B):
        raise ValueError("theta must be a float32 CUDA tensor [B,6] or [B,8]")
    tdim = theta.numel() // B
    entry, head = _with_interp("vstab_st_transform_backward", (img.data_ptr(), B, H, W, C, theta.data_ptr(), tdim), ip)
    return _backward_with_param_grad(entry, head, dout, (oh, ow), d_img, acc, need_img, need_theta, (B, tdim),
                                     "vstab_st_transform_backward_workspace_bytes", (B, H, W, C, oh, ow))


_SYM_THETA_DIM = {0: 6, 1: 8, 2: 4}          # VSTAB_SYM_AFFINE, _PROJECTIVE, _SIMILARITY


def st_symmetry_transform_backward(img, theta, dout, out_size, kind, need_img: bool = True, need_theta: bool = True, d_img=None,
                                   interp='bilinear'):
    """Gradients of SimilarityTransformer (kind 2) / AffineSymmetryTransformer (0) / ProjectiveSymmetryTransformer (1) .transform with
    the sampler `interp`, for the output gradient dout in the forward's output layout [B,ow,oh,C] (out_size = (oh, ow)): (d img
    [B,H,W,C] or None, d theta [B,4|6|8] or None).  H, W >= 100.  d_img, need_img, need_theta as in st_transform_backward; d img is
    summed by float atomics (its last bits may differ between runs), d theta is bit-reproducible.  The affine kind's pre-map
    multiplies theta by 0: its d theta is exactly zero for finite gradients.  The similarity kind's d theta couples the samples of a
    batch for B > 1, as the reference's interleave does."""
    ip = _st_interp(interp)
    kind = int(kind)
    if kind not in _SYM_THETA_DIM:
        raise ValueError("kind must be 0 (affine), 1 (projective) or 2 (similarity)")
    need_img = need_img or d_img is not None
    img, dout, (B, H, W, C, oh, ow), d_img, acc = _st_backward_args(img, dout, out_size, d_img, need_img)
    if H < 100 or W < 100:
        raise ValueError(f"the 100-pixel symmetric pad needs H, W >= 100, got {H}x{W}")
    tdim = _SYM_THETA_DIM[kind]
    theta = theta.contiguous()
    if not theta.is_cuda or theta.dtype != torch.float32 or theta.numel() != tdim * B:
        raise ValueError(f"theta must be a float32 CUDA tensor [B,{tdim}]")
    entry, head = _with_interp("vstab_st_symmetry_transform_backward", (img.data_ptr(), B, H, W, C, theta.data_ptr(), kind), ip)
    return _backward_with_param_grad(entry, head, dout, (oh, ow), d_img, acc, need_img, need_theta, (B, tdim),
                                     "vstab_st_symmetry_transform_backward_workspace_bytes", (B, H, W, C, oh, ow))


def st_elastic_transform_backward(img, theta, dout, out_size, g, linv_t, need_img: bool = True, need_theta: bool = True, d_img=None,
                                  interp='bilinear'):
    """Gradients of ElasticTransformer.transform (thin-plate spline, sampler `interp`) for the output gradient dout [B,oh,ow,C]:
    (d img [B,H,W,C] or None, d theta [B, 2*g*g] or None).  g is the control grid's side, linv_t the transformer's device table
    [g*g, g*g+3] (ElasticTransformer.L_inv).  d_img, need_img, need_theta as in st_transform_backward; d img is summed by float
    atomics (its last bits may differ between runs), d theta is bit-reproducible."""
    ip = _st_interp(interp)
    need_img = need_img or d_img is not None
    img, dout, (B, H, W, C, oh, ow), d_img, acc = _st_backward_args(img, dout, out_size, d_img, need_img)
    g = int(g)
    K = g * g
    theta = theta.contiguous()
    if not theta.is_cuda or theta.dtype != torch.float32 or theta.numel() != 2 * K * B:
        raise ValueError(f"theta must be a float32 CUDA tensor [B, {2 * K}]")
    if not torch.is_tensor(linv_t) or linv_t.device != img.device or linv_t.dtype != torch.float32 or linv_t.numel() != K * (K + 3):
        raise ValueError(f"linv_t must be a float32 tensor [{K}, {K + 3}] beside img")
    linv_t = linv_t.contiguous()
    entry, head = _with_interp("vstab_st_elastic_transform_backward", (img.data_ptr(), B, H, W, C, theta.data_ptr(), g, linv_t.data_ptr()), ip)
    return _backward_with_param_grad(entry, head, dout, (oh, ow), d_img, acc, need_img, need_theta, (B, 2 * K),
                                     "vstab_st_elastic_transform_backward_workspace_bytes", (B, H, W, C, g, oh, ow))


def st_bilinear_interp_backward(img, x, y, dout, out_size, need_img: bool = True, need_x: bool = True, need_y: bool = True, d_img=None):
    """Gradients of bilinear_interp(img, x, y, out_size) for dout [B*oh*ow, C]: (d img or None, d x [B*oh*ow] or None, d y or None);
    d_img as in st_transform_backward."""
    return _st_interp_backward("vstab_st_bilinear_interp_backward", img, x, y, dout, out_size, need_img, need_x, need_y, d_img)


def st_bicubic_interp_backward(img, x, y, dout, out_size, need_img: bool = True, need_x: bool = True, need_y: bool = True, d_img=None):
    """Gradients of bicubic_interp(img, x, y, out_size), arguments and results as st_bilinear_interp_backward.  d x, d y are zero
    where a coordinate is outside [-1, 1] or NaN (the clip), and reproducible; d img is summed by float atomics."""
    return _st_interp_backward("vstab_st_bicubic_interp_backward", img, x, y, dout, out_size, need_img, need_x, need_y, d_img)


def _st_interp_backward(entry, img, x, y, dout, out_size, need_img, need_x, need_y, d_img):
    need_img = need_img or d_img is not None
    img, dout, (B, H, W, C, oh, ow), d_img, acc = _st_backward_args(img, dout, out_size, d_img, need_img)
    x, y = x.contiguous().reshape(-1), y.contiguous().reshape(-1)
    for t in (x, y):
        if not t.is_cuda or t.dtype != torch.float32 or t.numel() != B * oh * ow:
            raise ValueError(f"x / y must be float32 CUDA tensors of B*out_h*out_w = {B * oh * ow} elements")
    d_x = torch.empty_like(x) if need_x else None
    d_y = torch.empty_like(y) if need_y else None
    runtime.call(img.device, entry, img.data_ptr(), B, H, W, C, x.data_ptr(), y.data_ptr(), dout.data_ptr(), oh, ow,
                 d_img.data_ptr() if need_img else None, 1 if acc else 0, _ptr(d_x), _ptr(d_y))
    return (d_img if need_img else None), d_x, d_y


def st3d_transform_backward(vol, theta, dout, out_size, need_vol: bool = True, need_theta: bool = True, d_vol=None):
    """Gradients of AffineVolumeTransformer.transform for the output gradient dout [B,od,oh,ow,C]: (d vol [B,D,H,W,C] or None,
    d theta [B,12] or None).  A given d_vol is added into, otherwise it is allocated and overwritten; need_vol / need_theta False
    skips that gradient's work.  d vol is summed by float atomics (its last bits may differ between runs); d theta is
    bit-reproducible."""
    need_vol = need_vol or d_vol is not None
    vol, dout, (B, D, H, W, C, od, oh, ow), d_vol, acc = _st_backward_args(vol, dout, out_size, d_vol, need_vol, rank=5)
    theta = theta.contiguous()
    if not theta.is_cuda or theta.dtype != torch.float32 or theta.numel() != 12 * B:
        raise ValueError("theta must be a float32 CUDA tensor [B,12]")
    return _backward_with_param_grad("vstab_st3d_transform_backward", (vol.data_ptr(), B, D, H, W, C, theta.data_ptr()), dout, (od, oh, ow),
                                     d_vol, acc, need_vol, need_theta, (B, 12), "vstab_st3d_transform_backward_workspace_bytes",
                                     (B, D, H, W, C, od, oh, ow))


def st3d_bilinear_interp_backward(vol, x, y, z, dout, out_size, edge_size: int = 1, need_vol: bool = True, need_x: bool = True,
                                  need_y: bool = True, need_z: bool = True, d_vol=None):
    """Gradients of bilinear_interp3d(vol, x, y, z, out_size, edge_size) for dout [B*od*oh*ow, C]: (d vol or None, d x [B*od*oh*ow]
    or None, d y or None, d z or None); d_vol as in st3d_transform_backward."""
    need_vol = need_vol or d_vol is not None
    vol, dout, (B, D, H, W, C, od, oh, ow), d_vol, acc = _st_backward_args(vol, dout, out_size, d_vol, need_vol, rank=5)
    x, y, z = x.contiguous().reshape(-1), y.contiguous().reshape(-1), z.contiguous().reshape(-1)
    for t in (x, y, z):
        if not t.is_cuda or t.dtype != torch.float32 or t.numel() != B * od * oh * ow:
            raise ValueError(f"x / y / z must be float32 CUDA tensors of B*out_d*out_h*out_w = {B * od * oh * ow} elements")
    d_x = torch.empty_like(x) if need_x else None
    d_y = torch.empty_like(y) if need_y else None
    d_z = torch.empty_like(z) if need_z else None
    runtime.call(vol.device, "vstab_st3d_bilinear_interp_backward", vol.data_ptr(), B, D, H, W, C, x.data_ptr(), y.data_ptr(), z.data_ptr(),
                 od, oh, ow, int(edge_size), dout.data_ptr(), d_vol.data_ptr() if need_vol else None, 1 if acc else 0,
                 _ptr(d_x), _ptr(d_y), _ptr(d_z))
    return (d_vol if need_vol else None), d_x, d_y, d_z


def homography_warp_backward(img, M, dout, out_size, need_img: bool = True, need_M: bool = True, d_img=None, ref=None):
    """Gradients of warp.warpImage (ref None: M [B,9] or [B,3,3] is the composed matrix) or of warp.transformImage / transformCropImage
    (ref [9] or [3,3] the refMtrx: M is pMtrx and the kernels compose ref . pMtrx as the forward does) for the output gradient dout
    [B,oh,ow,C]: (d img [B,Hi,Wi,C] or None, d M -- with ref: d pMtrx = ref^T . d (ref . pMtrx) -- [B,3,3] or None).  d_img, need_img
    as in st_transform_backward; need_M False skips the matrix gradient's work.  d img is summed by float atomics (its last bits may
    differ between runs); the matrix gradient is bit-reproducible.  ref gets no gradient."""
    need_img = need_img or d_img is not None
    img, dout, (B, H, W, C, oh, ow), d_img, acc = _st_backward_args(img, dout, out_size, d_img, need_img)
    if not torch.is_tensor(M) or M.device != img.device or M.dtype != torch.float32 or M.numel() != 9 * B:
        raise ValueError("M must be a float32 tensor [B,9] or [B,3,3] beside img")
    M = M.contiguous()
    if ref is None:
        entry, head = "vstab_homography_warp_backward", (img.data_ptr(), B, H, W, C, M.data_ptr())
    else:
        if not torch.is_tensor(ref) or ref.device != img.device or ref.dtype != torch.float32 or ref.numel() != 9:
            raise ValueError("ref must be a float32 tensor of 9 elements beside img")
        ref = ref.contiguous()
        entry, head = "vstab_transform_image_backward", (img.data_ptr(), B, H, W, C, ref.data_ptr(), M.data_ptr())
    return _backward_with_param_grad(entry, head, dout, (oh, ow), d_img, acc, need_img, need_M, (B, 3, 3),
                                     "vstab_homography_warp_backward_workspace_bytes", (B, H, W, C, oh, ow))


def vec2mtrx_backward(p, d_out, warp_type, warp_approx):
    """Gradient of warp.vec2mtrx: p [B,8] (warp_type 'homography') or [B,6] ('affine'), d_out [B,3,3] the gradient of the matrix ->
    d p of p's shape.  In double from the fp32 p, rounded once; bit-reproducible."""
    dim = {"homography": 8, "affine": 6}.get(warp_type)
    if dim is None:
        raise ValueError("warp_type must be 'homography' or 'affine'")
    p = runtime.f32_cuda(p, "p", 2, dim, f"[B,{dim}]")
    B = p.shape[0]
    if not torch.is_tensor(d_out) or d_out.device != p.device or d_out.dtype != torch.float32 or d_out.numel() != 9 * B:
        raise ValueError("d_out must be a float32 tensor [B,3,3] beside p")
    d_out = d_out.contiguous()
    d_p = torch.empty_like(p)
    runtime.call(p.device, "vstab_vec2mtrx_backward", p.data_ptr(), B, dim, int(warp_approx), d_out.data_ptr(), d_p.data_ptr())
    return d_p


def warp_flow_backward(img, flow, dout, need_img: bool = True, need_flow: bool = True, d_img=None):
    """Gradients of warp_flow.tf_warp(img [B,H,W,C], flow [B,H,W,2]) for the output gradient dout [B,H,W,C]: (d img [B,H,W,C] or None,
    d flow [B,H,W,2] or None) -- what TensorFlow's autodiff yields: the corner indices carry no gradient, the flow enters through the
    four weights of the clipped corners only.  d_img, need_img as in st_transform_backward; need_flow False skips the flow gradient's
    work.  d img is summed by float atomics (its last bits may differ between runs); d flow is bit-reproducible."""
    need_img = need_img or d_img is not None
    if not need_img and not need_flow:
        return None, None
    if not torch.is_tensor(img) or img.dim() != 4:
        raise ValueError("img must be a float32 CUDA tensor [B,H,W,C]")
    img, dout, (B, H, W, C, _, _), d_img, acc = _st_backward_args(img, dout, img.shape[1:3], d_img, need_img)
    if not torch.is_tensor(flow) or flow.device != img.device or flow.dtype != torch.float32 or tuple(flow.shape) != (B, H, W, 2):
        raise ValueError(f"flow must be a float32 tensor [{B},{H},{W},2] beside img")
    flow = flow.contiguous()
    d_flow = torch.empty_like(flow) if need_flow else None
    runtime.call(img.device, "vstab_warp_flow_backward", img.data_ptr(), flow.data_ptr(), dout.data_ptr(), B, H, W, C,
                 d_img.data_ptr() if need_img else None, _ptr(d_flow), 1 if acc else 0)
    return (d_img if need_img else None), d_flow


def get_pixel_value_backward(dout, x, y, img_hw, d_img=None):
    """Gradient of warp_flow.get_pixel_value with respect to its image: dout [B,H,W,C] scattered into d img [B,Hi,Wi,C] (img_hw =
    (Hi, Wi)) at the forward's clipped indices x, y (int32 [B,H,W]).  A given d_img is added into.  Float atomics: where several
    indices meet, the last bits depend on the arrival order."""
    dout = runtime.f32_cuda(dout, "dout", 4, layout="[B,H,W,C]")
    B, H, W, C = dout.shape
    if tuple(x.shape) != (B, H, W) or tuple(y.shape) != (B, H, W):
        raise ValueError(f"x and y must both be [{B},{H},{W}]")
    x = x.to(device=dout.device, dtype=torch.int32).contiguous()
    y = y.to(device=dout.device, dtype=torch.int32).contiguous()
    Hi, Wi = int(img_hw[0]), int(img_hw[1])
    acc = d_img is not None
    if acc and (tuple(d_img.shape) != (B, Hi, Wi, C) or d_img.dtype != torch.float32 or d_img.device != dout.device or not d_img.is_contiguous()):
        raise ValueError(f"d_img must be a contiguous float32 tensor [{B},{Hi},{Wi},{C}] beside dout")
    if d_img is None:
        d_img = torch.empty((B, Hi, Wi, C), dtype=torch.float32, device=dout.device)
    runtime.call(dout.device, "vstab_get_pixel_value_backward", dout.data_ptr(), x.data_ptr(), y.data_ptr(), d_img.data_ptr(), B, H, W, C,
                 Hi, Wi, 1 if acc else 0)
    return d_img


def flow_resize_scale_backward(dout, in_hw, net_h: int, net_w: int):
    """Gradient of warp_flow.flow_to_output_res with respect to predict_flow2 [B,h,w,2] (in_hw = (h, w)) for the gradient dout
    [B,oh,ow,2] of the output-resolution flow: (net_h / h) * resize^T(dout * (ow / net_w, oh / net_h)), one gain per channel.  A
    gather in a fixed order: bit-reproducible."""
    dout = runtime.f32_cuda(dout, "dout", 4, 2, "[B,oh,ow,2]")
    B, oh, ow, _ = dout.shape
    h, w = int(in_hw[0]), int(in_hw[1])
    d_flow = torch.empty((B, h, w, 2), dtype=torch.float32, device=dout.device)
    runtime.call(dout.device, "vstab_flow_resize_scale_backward", dout.data_ptr(), B, oh, ow, d_flow.data_ptr(), h, w, int(net_h), int(net_w))
    return d_flow


def resize_bilinear_backward(dout, in_hw, gain: float = 1.0, din=None):
    """din (+)= gain * adjoint of tf.image.resize_images(., dout's size) applied to dout [B,oh,ow,C]."""
    dout = dout.contiguous()
    B, oh, ow, C = dout.shape
    acc = din is not None
    if din is None:
        din = torch.empty((B, int(in_hw[0]), int(in_hw[1]), C), dtype=torch.float32, device=dout.device)
    runtime.call(dout.device, "vstab_resize_bilinear_backward", dout.data_ptr(), B, oh, ow, C, din.data_ptr(), din.shape[1], din.shape[2],
                 float(gain), 1 if acc else 0)
    return din
