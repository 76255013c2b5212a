"""Drop-ins for the flow visualisation at the end of each of the reference's main scripts: `flow_to_image`, `compute_color` and
`make_color_wheel` (main_flownetS_pyramid.py:824-957, the Middlebury colour code).  The colouring runs in two HIP launches
(csrc/flow_vis_ops.hip, C ABI `vstab_flow_to_image` in include/vstab.h) on the current stream, without a host synchronisation and
without atomics, so a flow that is already on the device -- `ClipStabiliser.last_outflow`, `NativeClipStabiliser.last_flows`,
`Trainer.forward_test` -- is coloured where it lies and two runs give the same bytes.  There is no CPU path: a NumPy array makes the
round trip through the device and comes back as NumPy arrays, so the reference's call sites work unchanged.

The arithmetic and its order are the reference's, because the colour is discontinuous at radius 1 (where the x0.75 branch starts)
and at the +-pi seam (where wheel row 55 meets row 1):
  * A pixel with |u| > 1e7 or |v| > 1e7 is *unknown*: it counts as (0,0) in the maximum and is drawn black.
  * Normalisation: the reference adds float64 eps to the float32 scalar `maxrad` and divides a float32 array by the sum.  Under the
    NumPy of the reference's day (value-based casting) that is a float32 division by `maxrad` itself, or by 2^-52 when `maxrad` is
    0.  That is the semantics kept here, whatever NumPy is installed:  d = maxrad > 0 ? maxrad : 2^-52,  un = u / d,  vn = v / d.
  * rad = sqrt(un*un + vn*vn), a = arctan2(-vn, -un) / pi, fk = (a + 1) / 2 * 54 + 1, k0 = floor(fk), k1 = k0 + 1 (56 wraps to 1),
    f = fk - k0, all in float32 with real negations (v = +0 gives -0, which decides the side of the seam a horizontal flow is on).
  * From there float64, as NumPy computes once float32 meets the float64 wheel:  col = (1-f) wheel[k0-1]/255 + f wheel[k1-1]/255,
    col = 1 - rad (1 - col) where rad <= 1 and 0.75 col elsewhere, byte = floor(255 col).
  * anglemap = uint8(a * 127 + 128) in float32, truncated, in all three channels.

Two departures from the reference are deliberate:
  * The caller's array is never modified.  The reference zeroes unknown pixels in the caller's array through a view.
  * A pixel with a NaN component is left out of the maximum (and drawn black; its anglemap value is 1, that of a zero flow).  In the
    reference one NaN makes `max(-1, np.max(rad))` come out as -1, an accident of argument order, and the whole image changes.

Beyond the reference: a batch `[B,H,W,2]` is coloured in one call, each sample normalised by its own largest radius as the
reference does for its single image, and `maxrad` fixes the normalisation instead (a float for all samples, or one value per
sample), which a video needs so that a colour means the same speed in every frame.  `return_maxrad=True` appends the radii used,
a float32 tensor or array `[B]` (`[1]` for a single image), to the result."""
from __future__ import annotations

import numpy as np
import torch

from . import runtime

_SEGMENTS = (15, 6, 4, 11, 13, 6)                   # RY, YG, GC, CB, BM, MR


def make_color_wheel():
    """The Middlebury colour wheel, a [55,3] float64 ndarray of values 0..255 (:910-957): six segments of 15, 6, 4, 11, 13 and 6
    rows; in each, one channel stays at 255 while another ramps up as floor(255 i / n) or down as 255 - floor(255 i / n)."""
    wheel = np.zeros((sum(_SEGMENTS), 3), dtype=np.float64)
    full = (0, 1, 1, 2, 2, 0)                       # the channel held at 255 in each segment ...
    ramp = (1, 0, 2, 1, 0, 2)                       # ... and the one that moves, up in even segments, down in odd ones
    row = 0
    for s, n in enumerate(_SEGMENTS):
        r = np.floor(255 * np.arange(n) / n)
        wheel[row:row + n, full[s]] = 255
        wheel[row:row + n, ramp[s]] = 255 - r if s % 2 else r
        row += n
    return wheel


def _run(flow: torch.Tensor, maxrad, want_anglemap: bool):
    """flow [B,H,W,2] float32 CUDA, contiguous; maxrad None or a [B] float32 CUDA tensor -> img, anglemap or None, radii [B]"""
    B, H, W, _ = flow.shape
    dev = flow.device
    if B * H * W == 0:
        raise ValueError(f"flow_to_image: empty flow {tuple(flow.shape)}")
    if flow.data_ptr() % 8:
        flow = flow.clone()                         # a view that starts inside a pixel
    img = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    ang = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev) if want_anglemap else None
    used = torch.empty((B,), dtype=torch.float32, device=dev)
    ws = runtime.workspace(dev, "vstab_flow_to_image_workspace_bytes", B, H, W) if maxrad is None else None
    runtime.call(dev, "vstab_flow_to_image", flow.data_ptr(), B, H, W, runtime.ptr(maxrad), img.data_ptr(), runtime.ptr(ang), used.data_ptr(),
                 runtime.ptr(ws), 0 if ws is None else ws.numel())
    return img, ang, used


def _radii(maxrad, B, device):
    if maxrad is None:
        return None
    if torch.is_tensor(maxrad) or isinstance(maxrad, np.ndarray):
        r = torch.as_tensor(maxrad).to(device=device, dtype=torch.float32).reshape(-1)
        if r.numel() == 1:
            r = r.expand(B)
        if r.numel() != B:
            raise ValueError(f"maxrad must be a float or hold one value per sample ({B}), got {r.numel()}")
        return r.contiguous()
    return torch.full((B,), float(maxrad), dtype=torch.float32, device=device)


def flow_to_image(flow, maxrad=None, anglemap=True, return_maxrad=False):
    """Middlebury colour image of a flow field (:824-864).  flow: [H,W,2] or [B,H,W,2], a float32 CUDA tensor (stays on the device,
    uint8 CUDA tensors come back; a non-dense one is made contiguous) or a NumPy array (NumPy arrays come back).  The input is never
    modified.  maxrad: None (each sample is normalised by its own largest radius), a float, or a tensor / array of one value per
    sample; a given radius is used as it is and no maximum is taken.  Returns (img, anglemap) as the reference does, img alone with
    anglemap=False; with return_maxrad=True the radii used, float32 [B], come last.  See the module docstring for the arithmetic
    and for the two deliberate departures from the reference (input untouched, NaN pixels left out of the maximum)."""
    as_numpy = isinstance(flow, np.ndarray)
    if as_numpy:
        runtime._require_gpu()
        t = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).cuda()
    elif torch.is_tensor(flow) and flow.is_cuda and flow.dtype == torch.float32:
        t = flow
    else:
        raise ValueError("flow must be a float32 CUDA tensor or a NumPy array, [H,W,2] or [B,H,W,2]")
    if t.dim() not in (3, 4) or t.shape[-1] != 2:
        raise ValueError(f"flow must be [H,W,2] or [B,H,W,2], got {tuple(t.shape)}")
    single = t.dim() == 3
    t4 = (t.unsqueeze(0) if single else t).contiguous()
    img, ang, used = _run(t4, _radii(maxrad, t4.shape[0], t4.device), bool(anglemap))
    out = [img, ang] if anglemap else [img]
    if single:
        out = [o[0] for o in out]
    if return_maxrad:
        out.append(used)
    if as_numpy:
        out = [o.cpu().numpy() for o in out]
    return out[0] if len(out) == 1 else tuple(out)


def compute_color(u, v):
    """Colours [H,W,3] uint8 of already normalised flow components u, v [H,W] (:867-908): flow_to_image with the radius fixed at 1,
    so nothing is divided.  Tensors or NumPy arrays, as flow_to_image; the inputs are not modified (the reference zeroes NaNs in
    place).  A component beyond 1e7 in magnitude marks the pixel unknown here as it does in flow_to_image, and draws it black."""
    if isinstance(u, np.ndarray) or isinstance(v, np.ndarray):
        flow = np.stack([np.asarray(u, dtype=np.float32), np.asarray(v, dtype=np.float32)], axis=-1)
    else:
        flow = torch.stack([u, v], dim=-1)
    if flow.ndim != 3:
        raise ValueError("compute_color takes u and v of shape [H,W]")
    return flow_to_image(flow, maxrad=1.0, anglemap=False)
