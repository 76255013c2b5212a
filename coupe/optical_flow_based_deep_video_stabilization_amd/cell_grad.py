"""Backward of cell.py's gate stages (csrc/cell_ops.hip), one thin wrapper per library entry point: `convlstm_gates_backward`,
`convgru_update_backward`, `convgru_gates_backward`.  cell.py's sequence functions string them together with `training.conv_wgrad` /
`conv_dgrad` (which is why they live beside cell.py and not in it: training re-exports them, and cell.py imports training)."""
from __future__ import annotations

import torch

from . import runtime
from .runtime import _up4, ptr as _ptr


def _cell_slice(t, name, shape):
    """a [B,H,W,F] float32 CUDA tensor that is contiguous or the channel slice of a wider NHWC buffer -> (address, channel stride)"""
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a float32 CUDA tensor {list(shape)}")
    _, H, W, _ = shape
    cs = t.stride(2)
    if t.stride(3) != 1 or cs < shape[3] or t.stride(1) != W * cs or t.stride(0) != H * W * cs:
        raise ValueError(f"{name} must be contiguous or a channel slice of a contiguous NHWC tensor")
    return t.data_ptr(), cs


def _cell_dense(t, name, shape=None):
    """a float32 CUDA tensor [B,H,W,F] (of the given shape when there is one), made contiguous"""
    t = runtime.f32_cuda(t, name, 4, layout=str(list(shape)) if shape is not None else "[B,H,W,F]")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a float32 CUDA tensor {list(shape)}")
    return t


def _cell_rows(y, name, channels):
    if not torch.is_tensor(y) or not y.is_cuda or y.dtype != torch.float32 or y.dim() != 4 or y.shape[3] < channels or not y.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 CUDA tensor [B,H,W,>={channels}]")
    return y


def _cell_param_grads(names_shapes, want, grads, accumulate, device):
    """the buffers the parameter gradients go to: those of `grads` (added to when accumulate), new ones otherwise; None when not wanted"""
    if not want:
        return {n: None for n in names_shapes}
    out = {}
    for n, s in names_shapes.items():
        t = None if grads is None else grads.get(n)
        if t is None:
            t = (torch.zeros if accumulate else torch.empty)(s, dtype=torch.float32, device=device)
        elif not t.is_cuda or t.dtype != torch.float32 or tuple(t.shape) != tuple(s) or not t.is_contiguous():
            raise ValueError(f"grads[{n!r}] must be a contiguous float32 CUDA tensor {list(s)}")
        out[n] = t
    return out


def convlstm_gates_backward(y, c, dh=None, dc_new=None, peepholes=None, gamma=None, beta=None, stats=None, forget_bias: float = 1.0, act: int = 0,
                            need_peepholes: bool = True, need_ln: bool = True, grads=None, accumulate: bool = False, dy=None):
    """Backward of what follows a ConvLSTMCell's convolution (`vstab_convlstm_gates_backward`).  y [B,H,W,>=4F] the convolution output, c
    [B,H,W,F] the old state, dh / dc_new the gradients of the returned h' (may be a channel slice) and c' (None = zero); peepholes
    (W_ci, W_cf, W_co) or None; gamma, beta [5,F] and stats = (the forward's [B,3,2] {mean, rstd} of j, i, f, its [B,2,2] of o, c') with
    normalize, else None.  Returns (dy [B,H,W,up4(4F)] = [dj, di, df, do] with zero pad channels, dc [B,H,W,F], grads) where grads has
    'W_ci', 'W_cf', 'W_co' [H,W,F] and 'gamma', 'beta' [5,F] (None where not wanted or not present); with `grads` given and accumulate
    the results are added to its tensors."""
    c = _cell_dense(c, "c")
    B, H, W, F = c.shape
    y = _cell_rows(y, "y", 4 * F)
    normalize, peephole = gamma is not None, peepholes is not None
    if normalize and (beta is None or stats is None):
        raise ValueError("normalize needs gamma, beta and the forward's statistics")
    dhp, dhs = _cell_slice(dh, "dh", c.shape) if dh is not None else (None, 0)
    dcn = _cell_dense(dc_new, "dc_new", c.shape) if dc_new is not None else None
    if dy is None:
        dy = torch.empty((B, H, W, _up4(4 * F)), dtype=torch.float32, device=c.device)
    _cell_rows(dy, "dy", 4 * F)
    dc = torch.empty_like(c)
    g = _cell_param_grads({n: (H, W, F) for n in ("W_ci", "W_cf", "W_co")}, peephole and need_peepholes, grads, accumulate, c.device)
    g.update(_cell_param_grads({"gamma": (5, F), "beta": (5, F)}, normalize and need_ln, grads, accumulate, c.device))
    ws = runtime.workspace(c.device, "vstab_convlstm_gates_backward_workspace_bytes", B, H, W, F, int(normalize), int(peephole))
    pe = [p.contiguous() for p in peepholes] if peephole else [None] * 3
    runtime.call(c.device, "vstab_convlstm_gates_backward",
                 y.data_ptr(), y.shape[3], c.data_ptr(), _ptr(pe[0]), _ptr(pe[1]), _ptr(pe[2]), _ptr(gamma), _ptr(beta),
                 _ptr(stats[0]) if normalize else None, _ptr(stats[1]) if normalize else None, dhp, dhs, _ptr(dcn), B, H, W, F, float(forget_bias),
                 int(act), int(normalize), int(peephole), dy.data_ptr(), dy.shape[3], dc.data_ptr(), _ptr(g["W_ci"]), _ptr(g["W_cf"]), _ptr(g["W_co"]),
                 _ptr(g["gamma"]), _ptr(g["beta"]), 1 if accumulate else 0, ws.data_ptr(), ws.numel())
    return dy, dc, g


def convgru_update_backward(y2, h, u, dh_new, gamma=None, beta=None, stats=None, act: int = 0, need_ln: bool = True, grads=None,
                            accumulate: bool = False, dy2=None, dh=None):
    """Backward of a ConvGRUCell's update stage (`vstab_convgru_update_backward`).  y2 [B,H,W,>=F] the candidate convolution's output, h the old
    state and dh_new the gradient of h' (either may be a channel slice), u [B,H,W,F]; gamma, beta [F] and stats (the forward's [B,1,2]) with
    normalize.  Returns (du [B,H,W,F], dy2 [B,H,W,up4(F)] with zero pad channels, dh = dh_new u -- written to `dh` when given, which may be a
    channel slice --, grads {'gamma', 'beta'})."""
    u = _cell_dense(u, "u")
    B, H, W, F = u.shape
    y2 = _cell_rows(y2, "y2", F)
    normalize = gamma is not None
    if normalize and (beta is None or stats is None):
        raise ValueError("normalize needs gamma, beta and the forward's statistics")
    hp, hs = _cell_slice(h, "h", u.shape)
    dnp, dns = _cell_slice(dh_new, "dh_new", u.shape)
    if dy2 is None:
        dy2 = torch.empty((B, H, W, _up4(F)), dtype=torch.float32, device=u.device)
    _cell_rows(dy2, "dy2", F)
    if dh is None:
        dh = torch.empty_like(u)
    dhp, dhs = _cell_slice(dh, "dh", u.shape)
    du = torch.empty_like(u)
    g = _cell_param_grads({"gamma": (F,), "beta": (F,)}, normalize and need_ln, grads, accumulate, u.device)
    ws = runtime.workspace(u.device, "vstab_convgru_backward_workspace_bytes", B, H, W, F, int(normalize))
    runtime.call(u.device, "vstab_convgru_update_backward", y2.data_ptr(), y2.shape[3], hp, hs, u.data_ptr(), _ptr(gamma), _ptr(beta),
                 _ptr(stats), dnp, dns, B, H, W, F, int(act), int(normalize), dy2.data_ptr(), dy2.shape[3], du.data_ptr(), dhp, dhs,
                 _ptr(g["gamma"]), _ptr(g["beta"]), 1 if accumulate else 0, ws.data_ptr(), ws.numel())
    return du, dy2, dh, g


def convgru_gates_backward(y, h, du, drh, dh, gamma=None, beta=None, stats=None, need_ln: bool = True, grads=None, accumulate: bool = False,
                           dy=None):
    """Backward of a ConvGRUCell's gates stage (`vstab_convgru_gates_backward`).  y [B,H,W,>=2F] the gates convolution's output, h the old state,
    du [B,H,W,F], drh the gradient of r h (h, drh and dh may be channel slices); gamma, beta [2,F] and stats (the forward's [B,2,2]) with
    normalize.  ADDS drh r to dh in place and returns (dy [B,H,W,up4(2F)] = [dr, du] with zero pad channels, grads {'gamma', 'beta'})."""
    du = _cell_dense(du, "du")
    B, H, W, F = du.shape
    y = _cell_rows(y, "y", 2 * F)
    normalize = gamma is not None
    if normalize and (beta is None or stats is None):
        raise ValueError("normalize needs gamma, beta and the forward's statistics")
    hp, hs = _cell_slice(h, "h", du.shape)
    rp, rs = _cell_slice(drh, "drh", du.shape)
    dhp, dhs = _cell_slice(dh, "dh", du.shape)
    if dy is None:
        dy = torch.empty((B, H, W, _up4(2 * F)), dtype=torch.float32, device=du.device)
    _cell_rows(dy, "dy", 2 * F)
    g = _cell_param_grads({"gamma": (2, F), "beta": (2, F)}, normalize and need_ln, grads, accumulate, du.device)
    ws = runtime.workspace(du.device, "vstab_convgru_backward_workspace_bytes", B, H, W, F, int(normalize))
    runtime.call(du.device, "vstab_convgru_gates_backward", y.data_ptr(), y.shape[3], hp, hs, _ptr(gamma), _ptr(beta), _ptr(stats),
                 du.data_ptr(), rp, rs, B, H, W, F, int(normalize), dy.data_ptr(), dy.shape[3], dhp, dhs, _ptr(g["gamma"]), _ptr(g["beta"]),
                 1 if accumulate else 0, ws.data_ptr(), ws.numel())
    return dy, g
