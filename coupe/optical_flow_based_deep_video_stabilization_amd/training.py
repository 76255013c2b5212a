"""Building blocks of the training step, one thin wrapper per library entry point: the objective
`lossterm` / `masked_MSE` (main:188-210, "main" = main_flownetS_pyramid_noprevloss_dataloader.py), the total-variation
terms and `loss_main` (main:213-275) with their gradient with respect to every predicted flow; filter / input gradients
of the conv and transposed-conv layers; BatchNorm(lrelu) in training mode and its backward; the padded nearest upsampling and its
adjoint.  `train_step.Trainer` strings them into the whole step (forward, loss, backward, Adam: main:184-185, 333-335).
The backward wrappers of everything else live beside what they differentiate and are re-exported here under their old names: the
samplers' in `sampler_grad`, SSIM's in `utils`, the recurrent cells' gate stages in `cell_grad`.
The objective of the reference's other two training scripts -- the same terms plus five weighted comparisons with earlier stabilised
frames -- is `Objective` / `lossterm_multi` / `loss_main_multi` (main_flownetS_pyramid.py:200-250).

Everything runs in the HIP library (csrc/train_ops.hip); there is no CPU path."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _lib, runtime
from .runtime import ptr as _ptr
from .warp_flow import resize_images
# the backward wrappers that moved beside what they differentiate, under the names they always had here
from .cell_grad import convgru_gates_backward, convgru_update_backward, convlstm_gates_backward  # noqa: F401
from .sampler_grad import (flow_resize_scale_backward, get_pixel_value_backward, homography_warp_backward,  # noqa: F401
                           resize_bilinear_backward, st3d_bilinear_interp_backward, st3d_transform_backward, st_bicubic_interp_backward,
                           st_bilinear_interp_backward, st_elastic_transform_backward, st_symmetry_transform_backward, st_transform_backward,
                           vec2mtrx_backward, warp_flow_backward)
from .utils import ssim_backward  # noqa: F401

LOSS_LEVELS = ("predict_flow6", "predict_flow5", "predict_flow4", "predict_flow3", "predict_flow2")
TV_WEIGHTS = (2e-8 * 3, 2e-8 * 3, 2e-8 * 3, 4e-8 * 1.5, 4e-8 * 1.5)          # main:269-273


def _f32(t, name, c):
    return runtime.f32_cuda(t, name, 4, c, f"[B,h,w,{c}]")


def _f32c(t, name):
    t = runtime.f32_cuda(t, name, 4, layout="[B,H,W,Ct], Ct >= 3")
    if t.shape[3] < 3:
        raise ValueError(f"{name} must be a float32 CUDA tensor [B,H,W,Ct], Ct >= 3")
    return t


def _level_inputs(predict_flow, targets, unstab_image, name, three: bool):
    """What lossterm and lossterm_multi do before their library call: the checked flow, the target tensor (`three`: exactly 3 channels,
    else Ct >= 3) and the unstable frame, both resized to the flow's size (tf.image.resize_images, main:202-203)."""
    pf = _f32(predict_flow, "predict_flow", 2)
    B, h, w, _ = pf.shape
    tg = _f32(targets, name, 3) if three else _f32c(targets, name)
    unstab = _f32(unstab_image, "unstab_image", 3)
    if tg.shape[0] != B or unstab.shape[:3] != tg.shape[:3]:
        raise ValueError(f"{name} / unstab_image must be [B,H,W,{3 if three else '.'}] with the flow's batch size")
    return pf, resize_images(tg, (h, w)), resize_images(unstab, (h, w))


def _level_descs(flows, grads, tv_weights, B):
    """The vstab_loss_level_desc array of loss_main_fused / loss_main_multi: one entry per LOSS_LEVELS name."""
    desc = (_lib.LossLevelDesc * len(LOSS_LEVELS))()
    for d, name, tvw in zip(desc, LOSS_LEVELS, tv_weights):
        pf = flows[name]
        if not pf.is_cuda or pf.dtype != torch.float32 or pf.dim() != 4 or pf.shape[0] != B or not pf.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float32 CUDA tensor [B,h,w,C]")
        d.pf, d.h, d.w, d.cs_pf, d.tv_weight = pf.data_ptr(), pf.shape[1], pf.shape[2], pf.shape[3], tvw
        if grads is not None:
            g = grads[name]
            if g.shape[:3] != pf.shape[:3] or g.dtype != torch.float32 or not g.is_contiguous() or g.device != pf.device:
                raise ValueError(f"grads[{name}] must be a contiguous float32 tensor [B,h,w,C'] beside the flow")
            d.grad, d.cs_grad = g.data_ptr(), g.shape[3]
    return desc


def lossterm(predict_flow, stab_image, unstab_image, tv_weight: float = 0.0, need_grad: bool = True):
    """main:200-210 (+ the level's TV term when tv_weight != 0).  Returns (loss [0-dim float64 CUDA tensor],
    d loss / d predict_flow [B,h,w,2] or None)."""
    pf, gt, un = _level_inputs(predict_flow, stab_image, unstab_image, "stab_image", three=True)
    B, h, w, _ = pf.shape
    sums = torch.empty(3 * B, dtype=torch.float64, device=pf.device)
    grad = torch.empty_like(pf) if need_grad else None
    runtime.call(pf.device, "vstab_loss_level", pf.data_ptr(), gt.data_ptr(), un.data_ptr(), B, h, w, sums.data_ptr(), 1.0, float(tv_weight),
                 _ptr(grad))
    s = sums.view(B, 3)
    loss = (s[:, 0] / s[:, 1]).mean() + tv_weight * s[:, 2].sum()
    return loss, grad


def loss_main(outputs: Dict[str, torch.Tensor], gtstab_image, unstab_image, need_grad: bool = True
              ) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """loss6+...+loss2 + var6+...+var2 (main:275) and its gradient w.r.t. each of the five flows."""
    total, grads = None, {}
    for name, tvw in zip(LOSS_LEVELS, TV_WEIGHTS):
        l, g = lossterm(outputs[name], gtstab_image, unstab_image, tvw, need_grad)
        total = l if total is None else total + l
        if need_grad:
            grads[name] = g
    return total, grads


def loss_main_fused(flows: Dict[str, torch.Tensor], gtstab_image, unstab_image, grads: Dict[str, torch.Tensor] = None):
    """loss_main and (optionally) its flow gradients through ONE library call (`vstab_loss_main`).  flows[name]: [B,h,w,C]
    float32 CUDA pixels whose channels 0..1 are the flow (C even; the Trainer keeps 4-channel pixels); grads[name] (if
    given): [B,h,w,C'] buffers whose channels 0..1 are overwritten.  Returns the loss as a 0-dim float64 CUDA tensor."""
    stab, unstab = _f32(gtstab_image, "stab_image", 3), _f32(unstab_image, "unstab_image", 3)
    B, H, W, _ = stab.shape
    if unstab.shape != stab.shape:
        raise ValueError("stab_image / unstab_image must have the same shape")
    desc = _level_descs(flows, grads, TV_WEIGHTS, B)
    ws = runtime.workspace(stab.device, "vstab_loss_main_workspace_bytes", desc, len(LOSS_LEVELS), B, refused=(
        "loss_main: bad level descriptors (channel counts must be even, level sizes below 2^31 / 3 pixels, B <= 65535)"))
    out = torch.empty((), dtype=torch.float64, device=stab.device)
    runtime.call(stab.device, "vstab_loss_main", desc, len(LOSS_LEVELS), stab.data_ptr(), unstab.data_ptr(), B, H, W, out.data_ptr(),
                 ws.data_ptr(), ws.numel())
    return out


# ----------------------------------------------------------------------------- the objective with the previous-frame terms
# main_flownetS_pyramid.py:214-242 writes the weights of the five previous-frame terms as np.exp(-1/3), np.exp(-2/3), np.exp(-3/3),
# np.exp(-6/3), np.exp(-14/3).  The script is Python 2 (print statements at :358-360) without `from __future__ import division`, so
# -1/3 is FLOOR division: -1, -1, -1, -2, -5.  Those are the weights its checkpoints were trained with, and the presets' weights.
PREV_WEIGHTS_PY2_FLOOR_DIVISION = (math.exp(-1.0), math.exp(-1.0), math.exp(-1.0), math.exp(-2.0), math.exp(-5.0))
# What the expressions would give under true division (Python 3 semantics): offered by name for whoever wants the weights as they
# read on the page; no preset uses them.
PREV_WEIGHTS_TRUE_DIVISION = (math.exp(-1.0 / 3.0), math.exp(-2.0 / 3.0), math.exp(-1.0), math.exp(-2.0), math.exp(-14.0 / 3.0))


@dataclass(frozen=True)
class Objective:
    """loss_main of one of the reference's training scripts: at every pyramid level (LOSS_LEVELS order)
    sum_t target_weights[t] * lossterm(flow, stab[..., target_channels[t] : +3], unstab) + tv_weights[level] * total_variation(flow).
    The weights are stated in double and rounded to float32 where the library's ABI carries float (as `tv_weight` always was).

    Presets: OBJECTIVE_NOPREV = main_flownetS_pyramid_noprevloss_dataloader.py, OBJECTIVE_PREV = main_flownetS_pyramid.py,
    OBJECTIVE_PREV_HIGHTV = main_flownetS_pyramid_highTV_noBBloss.py.  The two prev presets weigh the five earlier frames with
    PREV_WEIGHTS_PY2_FLOOR_DIVISION = exp(-1), exp(-1), exp(-1), exp(-2), exp(-5): the scripts write np.exp(-1/3) ... np.exp(-14/3)
    and run under Python 2, where -1/3 floors to -1 and -14/3 to -5, so these are the values their checkpoints were trained with.
    PREV_WEIGHTS_TRUE_DIVISION = exp(-1/3), exp(-2/3), exp(-1), exp(-2), exp(-14/3) is what the same text means under true
    division; pass it to `with_target_weights` to get that variant.  Level 4's TV weight is 0 in both prev presets: the scripts
    compute var4 but leave it out of the sum."""
    target_channels: Tuple[int, ...]
    target_weights: Tuple[float, ...]
    tv_weights: Tuple[float, ...]

    def __post_init__(self):
        if not 1 <= len(self.target_channels) <= 8 or len(self.target_weights) != len(self.target_channels):
            raise ValueError("an Objective has 1..8 targets, one weight each")
        if len(self.tv_weights) != len(LOSS_LEVELS):
            raise ValueError(f"an Objective has {len(LOSS_LEVELS)} TV weights (levels 6, 5, 4, 3, 2)")

    def with_target_weights(self, prev_weights):
        """The same objective with other weights on the targets after the first (e.g. PREV_WEIGHTS_TRUE_DIVISION)."""
        return Objective(self.target_channels, (self.target_weights[0],) + tuple(float(v) for v in prev_weights), self.tv_weights)


# main_flownetS_pyramid_noprevloss_dataloader.py: the ground-truth frame only (what loss_main / loss_main_fused compute)
OBJECTIVE_NOPREV = Objective((0,), (1.0,), TV_WEIGHTS)
_PREV_CHANNELS = (0, 3, 6, 9, 12, 15)                           # stab_image[..., 0:3] and the five earlier frames :203-241
# main_flownetS_pyramid.py: TV / 2e7 on every level (:244-248), var4 computed (:246) but left out of the sum (:250) -> weight 0
OBJECTIVE_PREV = Objective(_PREV_CHANNELS, (1.0,) + PREV_WEIGHTS_PY2_FLOOR_DIVISION, (1 / 2e7, 1 / 2e7, 0.0, 1 / 2e7, 1 / 2e7))
# main_flownetS_pyramid_highTV_noBBloss.py: TV / 1e6 on levels 6, 5, (4), / 2e6 on levels 3, 2; var4 left out there too
OBJECTIVE_PREV_HIGHTV = Objective(_PREV_CHANNELS, (1.0,) + PREV_WEIGHTS_PY2_FLOOR_DIVISION, (1 / 1e6, 1 / 1e6, 0.0, 1 / 2e6, 1 / 2e6))
OBJECTIVES = {"noprev": OBJECTIVE_NOPREV, "prev": OBJECTIVE_PREV, "prev_hightv": OBJECTIVE_PREV_HIGHTV}


def _targets(c_off, weights, Ct):
    c_off, weights = [int(v) for v in c_off], [float(v) for v in weights]
    T = len(c_off)
    if not 1 <= T <= 8 or len(weights) != T:
        raise ValueError("1..8 targets, one weight each")
    if any(o < 0 or o + 3 > Ct for o in c_off):
        raise ValueError(f"every target needs its 3 channels inside the {Ct} channels of the target tensor")
    return T, (C.c_int32 * T)(*c_off), (C.c_float * T)(*weights), weights


def lossterm_multi(predict_flow, targets, unstab_image, c_off, weights, tv_weight: float = 0.0, need_grad: bool = True):
    """One level of main_flownetS_pyramid.py:203-250: sum_t weights[t] * lossterm(predict_flow, targets[..., c_off[t]:c_off[t]+3],
    unstab_image) + tv_weight * TV in one kernel pair (`vstab_loss_level_multi`): the warp, the mask and the denominator are shared.
    targets [B,H,W,Ct] is resized once, all channels.  Returns (loss [0-dim float64 CUDA tensor], d loss / d predict_flow [B,h,w,2]
    or None, per-target lossterms [T] float64, unweighted)."""
    pf, gt, un = _level_inputs(predict_flow, targets, unstab_image, "targets", three=False)
    B, h, w, _ = pf.shape
    Ct = gt.shape[3]
    T, offs, wts, _w = _targets(c_off, weights, Ct)
    sums = torch.empty((T + 2) * B, dtype=torch.float64, device=pf.device)
    grad = torch.empty_like(pf) if need_grad else None
    runtime.call(pf.device, "vstab_loss_level_multi", pf.data_ptr(), gt.data_ptr(), Ct, T, offs, wts, un.data_ptr(), B, h, w, sums.data_ptr(),
                 float(tv_weight), _ptr(grad))
    s = sums.view(B, T + 2)
    per = (s[:, :T] / s[:, T:T + 1]).mean(dim=0)
    tvw32 = float(torch.tensor(float(tv_weight), dtype=torch.float32))            # as the kernel and vstab_loss_main_multi carry it
    loss = (per * torch.tensor(list(wts), dtype=torch.float64, device=pf.device)).sum() + tvw32 * s[:, T + 1].sum()
    return loss, grad, per


def loss_main_multi(flows: Dict[str, torch.Tensor], stab_image, unstab_image, objective: Objective, grads: Dict[str, torch.Tensor] = None):
    """loss_main of `objective` and (optionally) its flow gradients through ONE library call (`vstab_loss_main_multi`).  stab_image:
    [B,H,W,Ct] (24 channels in the scripts; any Ct that holds the objective's targets); flows / grads as in loss_main_fused.
    Returns (loss, per-target lossterms summed over the levels [T], unweighted), float64 CUDA tensors."""
    stab, unstab = _f32c(stab_image, "stab_image"), _f32(unstab_image, "unstab_image", 3)
    B, H, W, Ct = stab.shape
    if unstab.shape[:3] != stab.shape[:3]:
        raise ValueError("stab_image / unstab_image must have the same batch and frame size")
    T, offs, wts, _w = _targets(objective.target_channels, objective.target_weights, Ct)
    desc = _level_descs(flows, grads, objective.tv_weights, B)
    ws = runtime.workspace(stab.device, "vstab_loss_main_multi_workspace_bytes", desc, len(LOSS_LEVELS), B, Ct, T, refused=(
        "loss_main_multi: the library rejects the level descriptors (1..8 levels, even channel counts >= 2, 8-byte aligned "
        "flow / gradient buffers, level sizes below 2^31 / 3 pixels)"))
    out = torch.empty(1 + T, dtype=torch.float64, device=stab.device)
    runtime.call(stab.device, "vstab_loss_main_multi", desc, len(LOSS_LEVELS), stab.data_ptr(), Ct, T, offs, wts, unstab.data_ptr(), B, H, W,
                 out.data_ptr(), ws.data_ptr(), ws.numel())
    return out[0], out[1:]


# ----------------------------------------------------------------------------- the test pass's report of the objective
@dataclass
class LossReport:
    """What the reference logs of loss_main on a batch (main:346-372), float64 CUDA tensors: `total` (0-dim; `loss_main_test`), `mse` and
    `tv` [5] in LOSS_LEVELS order (the summary scalars loss6..loss2 and var6..var2; total = mse.sum() + tv.sum() up to the last bit),
    `per_target` [T] (unweighted, summed over the levels, as loss_main_multi returns them) and `warped`: {level: warpedimgN [B,h,w,3]},
    float32 or the uint8 `fix_image_tf(warpedimgN, 1)` of the image log, or None when no previews were asked for."""
    total: torch.Tensor
    mse: torch.Tensor
    tv: torch.Tensor
    per_target: torch.Tensor
    warped: Optional[Dict[str, torch.Tensor]]


_PREVIEW_DTYPES = {"float32": (0, torch.float32), "uint8": (1, torch.uint8)}


def loss_report(flows: Dict[str, torch.Tensor], stab_image, unstab_image, objective: Objective = None, previews: str = None, *,
                preview_levels=None) -> LossReport:
    """loss_main of `objective` with its terms level by level and, on request, lossterm's second return value `warpedimg` of every
    level, through ONE library call without a gradient pass (`vstab_loss_report`): what the reference's test pass and summaries read
    (main:277-326, 346-372).  flows as loss_main_fused takes them (the Trainer's 4-channel pixels included).  objective None:
    OBJECTIVE_NOPREV on a 3-channel stab_image; otherwise stab_image is the multi-channel stable tensor of loss_main_multi.
    previews: None, 'uint8' (`utils.fix_image_tf(warpedimg, 1)`) or 'float32'; preview_levels: the LOSS_LEVELS names to store (all when
    None) -- a level left out runs the kernel without the store.  `total` and `per_target` are what loss_main_fused / loss_main_multi
    return on the same inputs.  Nothing is synchronised."""
    unstab = _f32(unstab_image, "unstab_image", 3)
    if objective is None:
        objective, stab = OBJECTIVE_NOPREV, _f32(stab_image, "stab_image", 3)
    else:
        stab = _f32c(stab_image, "stab_image")
    B, H, W, Ct = stab.shape
    if unstab.shape[:3] != stab.shape[:3]:
        raise ValueError("stab_image / unstab_image must have the same batch and frame size")
    if previews is not None and previews not in _PREVIEW_DTYPES:
        raise ValueError("previews must be None, 'uint8' or 'float32'")
    T, offs, wts, _w = _targets(objective.target_channels, objective.target_weights, Ct)
    desc = _level_descs(flows, None, objective.tv_weights, B)
    nl = len(LOSS_LEVELS)
    warped, ptrs, code = None, None, 0
    if previews is not None:
        code, dtype = _PREVIEW_DTYPES[previews]
        names = LOSS_LEVELS if preview_levels is None else tuple(preview_levels)
        if not set(names) <= set(LOSS_LEVELS):
            raise ValueError(f"preview_levels must be among {LOSS_LEVELS}")
        warped = {k: torch.empty((B, flows[k].shape[1], flows[k].shape[2], 3), dtype=dtype, device=stab.device) for k in LOSS_LEVELS if k in names}
        ptrs = (C.c_void_p * nl)(*[warped[k].data_ptr() if k in warped else None for k in LOSS_LEVELS])
    ws = runtime.workspace(stab.device, "vstab_loss_report_workspace_bytes", desc, nl, B, Ct, T, refused=(
        "loss_report: the library rejects the level descriptors (even channel counts >= 2, 8-byte aligned flows, level "
        "sizes below 2^31 / 3 pixels, B <= 65535)"))
    out = torch.empty(1 + T + 2 * nl, dtype=torch.float64, device=stab.device)
    runtime.call(stab.device, "vstab_loss_report", desc, nl, stab.data_ptr(), Ct, T, offs, wts, unstab.data_ptr(), B, H, W, ptrs, code,
                 out.data_ptr(), ws.data_ptr(), ws.numel())
    return LossReport(out[0], out[1 + T:1 + T + nl], out[1 + T + nl:], out[1:1 + T], warped)


# ----------------------------------------------------------------------------- backward building blocks
def conv_wgrad(x, gout, k: int, stride: int, pad: int, cx_off: int = 0, cin: int = None, cg_off: int = 0, cout: int = None,
               dW=None, db=None, accumulate: bool = False, want_db: bool = True):
    """Filter and bias gradient of PadLayer(pad) -> Conv2d(k, stride, VALID) (model.py:807-844): what TF's autodiff
    returns for tf.nn.conv2d's filter, in the reference's HWIO layout.  x [B,Hi,Wi,Cs_x] (channels cx_off..+cin),
    gout [B,Ho,Wo,Cs_g] (channels cg_off..+cout).  Returns (dW [k,k,cin,cout], db [cout] or None)."""
    x, gout = (runtime.f32_cuda(t, name, 4, layout="[B,H,W,C]") for t, name in ((x, "x"), (gout, "gout")))
    B, Hi, Wi, cs_x = x.shape
    _, Ho, Wo, cs_g = gout.shape
    cin = cs_x - cx_off if cin is None else int(cin)
    cout = cs_g - cg_off if cout is None else int(cout)
    if gout.shape[0] != B:
        raise ValueError("x and gout must have the same batch size")
    if dW is None:
        dW = torch.empty((k, k, cin, cout), dtype=torch.float32, device=x.device)
        accumulate = False
    if want_db and db is None:
        db = torch.empty((cout,), dtype=torch.float32, device=x.device)
    ws = runtime.workspace(x.device, "vstab_conv_wgrad_workspace_bytes", B, Ho, Wo, k, cin, cout)
    runtime.call(x.device, "vstab_conv_wgrad", x.data_ptr(), B, Hi, Wi, cs_x, cx_off, cin, gout.data_ptr(), Ho, Wo, cs_g, cg_off, cout,
                 k, stride, pad, dW.data_ptr(), db.data_ptr() if want_db else None, 1 if accumulate else 0, ws.data_ptr(), ws.numel())
    return dW, (db if want_db else None)


def conv_dgrad(gout, W, stride: int, pad: int, in_hw, cg_off: int = 0, cout: int = None, dx=None, cx_off: int = 0,
               accumulate: bool = False, bias=None):
    """Input gradient of PadLayer(pad) -> Conv2d(k, stride, VALID) with filter W [k,k,cin,cout] (CUDA tensor, HWIO):
    what TF's autodiff returns for tf.nn.conv2d's input.  gout [B,Ho,Wo,Cs_g] (channels cg_off..+cout); the result has
    the input's size in_hw and lands in channels cx_off..+cin of dx (allocated [B,Hi,Wi,cin] when None)."""
    gout, W = runtime.f32_cuda(gout, "gout", 4, layout="[B,Ho,Wo,C]"), runtime.f32_cuda(W, "W", 4, layout="[k,k,cin,cout]")
    if W.shape[0] != W.shape[1]:
        raise ValueError("W must be a float32 CUDA tensor [k,k,cin,cout]")
    B, Ho, Wo, cs_g = gout.shape
    k, _, cin, cout_w = W.shape
    cout = cout_w if cout is None else int(cout)
    if cout != cout_w:
        raise ValueError("cout must match the filter")
    Hi, Wi = int(in_hw[0]), int(in_hw[1])
    if dx is None:
        dx = torch.empty((B, Hi, Wi, cin), dtype=torch.float32, device=gout.device)
        accumulate, cx_off = False, 0
    cs_x = dx.shape[3]
    ws = runtime.workspace(gout.device, "vstab_conv_dgrad_workspace_bytes", B, Ho, Wo, cs_g, cout, k, stride, pad, Hi, Wi, cs_x, cx_off, cin,
                           1 if accumulate else 0,
                           refused="conv_dgrad: unsupported geometry (stride 1 or 2, channel counts multiples of 4, matching sizes)")
    runtime.call(gout.device, "vstab_conv_dgrad", gout.data_ptr(), B, Ho, Wo, cs_g, cg_off, cout, W.data_ptr(), _ptr(bias), k, stride, pad,
                 dx.data_ptr(), Hi, Wi, cs_x, cx_off, cin, 1 if accumulate else 0, ws.data_ptr(), ws.numel())
    return dx


def _rows_view(t, c_off, C):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous():
        raise ValueError("expected a contiguous float32 CUDA tensor [B,H,W,C]")
    cs = t.shape[3]
    C = cs - c_off if C is None else int(C)
    return t.shape[0] * t.shape[1] * t.shape[2], cs, C


def bn_lrelu_train_forward(z, beta, moving_mean=None, moving_var=None, decay: float = 0.9, eps: float = 1e-5, c_off: int = 0, C: int = None):
    """BatchNormLayer(act=lrelu 0.1, is_train=True, gamma_init=None) IN PLACE on channels c_off..+C of z (model.py:809 etc.):
    z is overwritten by y; moving_mean / moving_var (if given) get TensorLayer's moving-average update.
    Returns (y (= z), save_mean, save_rstd)."""
    rows, cs, C = _rows_view(z, c_off, C)
    mean = torch.empty(C, dtype=torch.float32, device=z.device)
    rstd = torch.empty(C, dtype=torch.float32, device=z.device)
    sc = runtime.workspace(z.device, "vstab_bn_scratch_bytes", rows, C)
    runtime.call(z.device, "vstab_bn_lrelu_train_forward", z.data_ptr(), rows, cs, c_off, C, beta.data_ptr(), _ptr(moving_mean), _ptr(moving_var),
                 float(decay), float(eps), mean.data_ptr(), rstd.data_ptr(), sc.data_ptr(), sc.numel())
    return z, mean, rstd


def bn_lrelu_inference_forward(z, beta, moving_mean, moving_var, eps: float = 1e-5, c_off: int = 0, C: int = None):
    """BatchNormLayer(act=lrelu 0.1, is_train=False, gamma_init=None) IN PLACE on channels c_off..+C of z: y = lrelu((z - moving_mean)
    * rsqrt(moving_var + eps) + beta).  The moving statistics are read only.  Returns y (= z)."""
    rows, cs, C = _rows_view(z, c_off, C)
    runtime.call(z.device, "vstab_bn_lrelu_inference_forward", z.data_ptr(), rows, cs, c_off, C, beta.data_ptr(), moving_mean.data_ptr(),
                 moving_var.data_ptr(), float(eps))
    return z


def bn_lrelu_train_backward(y, dy, beta, save_rstd, cy_off: int = 0, cg_off: int = 0, C: int = None, dbeta=None, accumulate: bool = False):
    """Backward of the layer above: dy (gradient w.r.t. y) is overwritten IN PLACE by the gradient w.r.t. the layer's input;
    returns (dz (= dy), dbeta)."""
    rows, cs_y, Cy = _rows_view(y, cy_off, C)
    rows_g, cs_g, Cg = _rows_view(dy, cg_off, C)
    if rows != rows_g or Cy != Cg:
        raise ValueError("y and dy must cover the same rows and channel count")
    if dbeta is None:
        dbeta = torch.empty(Cy, dtype=torch.float32, device=y.device)
        accumulate = False
    sc = runtime.workspace(y.device, "vstab_bn_scratch_bytes", rows, Cy)
    runtime.call(y.device, "vstab_bn_lrelu_train_backward", y.data_ptr(), cs_y, cy_off, dy.data_ptr(), cs_g, cg_off, Cy, rows, beta.data_ptr(),
                 save_rstd.data_ptr(), dbeta.data_ptr(), 1 if accumulate else 0, sc.data_ptr(), sc.numel())
    return dy, dbeta


def lrelu_backward(y, dy, cy_off: int = 0, cg_off: int = 0, C: int = None):
    """dy *= (y > 0 ? 1 : 0.1) in place."""
    rows, cs_y, Cy = _rows_view(y, cy_off, C)
    _, cs_g, _ = _rows_view(dy, cg_off, C)
    runtime.call(y.device, "vstab_lrelu_backward", y.data_ptr(), cs_y, cy_off, dy.data_ptr(), cs_g, cg_off, Cy, rows)
    return dy


def pad_nearest_upsample(src, H: int, W: int):
    """PadLayer(1) -> nearest resize (align_corners=True) to HxW (model.py:795-802, 882-884); C % 4 == 0."""
    src = src.contiguous()
    B, h2, w2, C = src.shape
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=src.device)
    runtime.call(src.device, "vstab_pad_nearest_upsample", src.data_ptr(), B, h2, w2, C, out.data_ptr(), H, W)
    return out


def pad_nearest_upsample_backward(dout, src_hw, dsrc=None):
    dout = dout.contiguous()
    B, H, W, C = dout.shape
    acc = dsrc is not None
    if dsrc is None:
        dsrc = torch.empty((B, int(src_hw[0]), int(src_hw[1]), C), dtype=torch.float32, device=dout.device)
    runtime.call(dout.device, "vstab_pad_nearest_upsample_backward", dout.data_ptr(), B, H, W, C, dsrc.data_ptr(), dsrc.shape[1], dsrc.shape[2],
                 1 if acc else 0)
    return dsrc


def conv3x3_winograd(x, W, transpose: bool = False, bias=None, y=None, cx_off: int = 0, cy_off: int = 0, act: int = 0):
    """3x3 stride-1 pad-1 convolution (transpose=False: x [..,cin] -> [..,cout]) or its input gradient (transpose=True:
    x = output gradient [..,cout] -> dx [..,cin]) in Winograd F(2x2,3x3) form; W [3,3,cin,cout] CUDA tensor.  act 0 none,
    1 leaky relu 0.1, 3 add to what is in y."""
    x, W = runtime.f32_cuda(x, "x", 4, layout="[B,H,W,C]"), W.contiguous()
    B, H, Wd, cs_x = x.shape
    cin, cout = int(W.shape[2]), int(W.shape[3])
    n_out = cin if transpose else cout
    if y is None:
        y = torch.empty((B, H, Wd, n_out), dtype=torch.float32, device=x.device)
        cy_off = 0
    ws = runtime.workspace(x.device, "vstab_conv3x3_winograd_workspace_bytes", B, H, Wd, cin, cout, 1 if transpose else 0, refused=(
        "conv3x3_winograd: unsupported geometry (reduction channels % 32, output channels % 64, < 2 GiB per tensor)"))
    runtime.call(x.device, "vstab_conv3x3_winograd", x.data_ptr(), B, H, Wd, cs_x, cx_off, W.data_ptr(), cin, cout, 1 if transpose else 0,
                 _ptr(bias), y.data_ptr(), y.shape[3], cy_off, act, ws.data_ptr(), ws.numel())
    return y


def conv3x3_winograd_wgrad(x, gout, cx_off: int = 0, cin: int = None, cg_off: int = 0, cout: int = None, dW=None):
    """Filter gradient of PadLayer(1) -> Conv2d(3, 1, VALID) (model.py:822, 829, 836, 843) in the Winograd domain
    (`vstab_conv3x3_winograd_wgrad`): same result as `conv_wgrad(x, gout, 3, 1, 1)` up to fp32 rounding at 4/9 of its
    multiply-adds.  x [B,H,W,Cs_x] (channels cx_off..+cin), gout [B,H,W,Cs_g] (channels cg_off..+cout) -> dW [3,3,cin,cout]."""
    x, gout = x.contiguous(), gout.contiguous()
    B, H, W, cs_x = x.shape
    cs_g = gout.shape[3]
    cin = cs_x - cx_off if cin is None else int(cin)
    cout = cs_g - cg_off if cout is None else int(cout)
    if gout.shape[:3] != x.shape[:3]:
        raise ValueError("gout must have the spatial size of x (stride 1, pad 1)")
    ws = runtime.workspace(x.device, "vstab_conv3x3_winograd_wgrad_workspace_bytes", B, H, W, cin, cout,
                           refused="conv3x3_winograd_wgrad: channel counts must be multiples of 4 (and tensors < 2 GiB)")
    if dW is None:
        dW = torch.empty((3, 3, cin, cout), dtype=torch.float32, device=x.device)
    runtime.call(x.device, "vstab_conv3x3_winograd_wgrad", x.data_ptr(), B, H, W, cs_x, cx_off, cin, gout.data_ptr(), cs_g, cg_off, cout,
                 dW.data_ptr(), ws.data_ptr(), ws.numel())
    return dW
