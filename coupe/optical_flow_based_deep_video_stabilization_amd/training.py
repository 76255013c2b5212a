"""Building blocks of the training step, one thin wrapper per library entry point: the objective
`lossterm` / `masked_MSE` (main:188-210, "main" = main_flownetS_pyramid_noprevloss_dataloader.py), the total-variation
terms and `loss_main` (main:213-275) with their gradient with respect to every predicted flow; filter / input gradients
of the conv and transposed-conv layers; BatchNorm(lrelu) in training mode and its backward; the resamplers' adjoints; the
gradients of the spatial transformers, bilinear and bicubic (`st_bicubic_interp_backward`, `st_transform_backward`, `st_symmetry_transform_backward`, `st_elastic_transform_backward`, `st_bilinear_interp_backward`)
and of warp.py's homography warp and matrix exponential (`homography_warp_backward`, `vec2mtrx_backward`), of utils.py's SSIM (`ssim_backward`)
and of cell.py's gate stages (`convlstm_gates_backward`, `convgru_update_backward`, `convgru_gates_backward`).
`train_step.Trainer` strings them into the whole step (forward, loss, backward, Adam: main:184-185, 333-335).
The objective of the reference's other two training scripts -- the same terms plus five weighted comparisons with earlier stabilised
frames -- is `Objective` / `lossterm_multi` / `loss_main_multi` (main_flownetS_pyramid.py:200-250).

Everything runs in the HIP library (csrc/train_ops.hip); there is no CPU path."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _lib, runtime
from .cell import _up4
from .warp_flow import resize_images

LOSS_LEVELS = ("predict_flow6", "predict_flow5", "predict_flow4", "predict_flow3", "predict_flow2")
TV_WEIGHTS = (2e-8 * 3, 2e-8 * 3, 2e-8 * 3, 4e-8 * 1.5, 4e-8 * 1.5)          # main:269-273


def _f32(t, name, c):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[3] != c:
        raise ValueError(f"{name} must be a float32 CUDA tensor [B,h,w,{c}]")
    return t.contiguous()


def _f32c(t, name):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[3] < 3:
        raise ValueError(f"{name} must be a float32 CUDA tensor [B,H,W,Ct], Ct >= 3")
    return t.contiguous()


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
    with torch.cuda.device(pf.device):
        _lib.check(_lib.lib().vstab_loss_level(pf.data_ptr(), gt.data_ptr(), un.data_ptr(), B, h, w, sums.data_ptr(), 1.0,
                                               float(tv_weight), grad.data_ptr() if need_grad else None, runtime.stream_ptr()))
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
    import ctypes as C
    stab, unstab = _f32(gtstab_image, "stab_image", 3), _f32(unstab_image, "unstab_image", 3)
    B, H, W, _ = stab.shape
    if unstab.shape != stab.shape:
        raise ValueError("stab_image / unstab_image must have the same shape")
    desc = _level_descs(flows, grads, TV_WEIGHTS, B)
    L = _lib.lib()
    n = L.vstab_loss_main_workspace_bytes(C.addressof(desc), len(LOSS_LEVELS), B)
    if n == 0:
        raise ValueError("loss_main: bad level descriptors (channel counts must be even, level sizes below 2^31 / 3 pixels, B <= 65535)")
    ws = torch.empty(n, dtype=torch.uint8, device=stab.device)
    out = torch.empty((), dtype=torch.float64, device=stab.device)
    with torch.cuda.device(stab.device):
        _lib.check(L.vstab_loss_main(C.addressof(desc), len(LOSS_LEVELS), stab.data_ptr(), unstab.data_ptr(), B, H, W, out.data_ptr(),
                                     ws.data_ptr(), n, runtime.stream_ptr()))
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
    import ctypes as C
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
    with torch.cuda.device(pf.device):
        _lib.check(_lib.lib().vstab_loss_level_multi(pf.data_ptr(), gt.data_ptr(), Ct, T, offs, wts, un.data_ptr(), B, h, w, sums.data_ptr(),
                                                     float(tv_weight), grad.data_ptr() if need_grad else None, runtime.stream_ptr()))
    s = sums.view(B, T + 2)
    per = (s[:, :T] / s[:, T:T + 1]).mean(dim=0)
    tvw32 = float(torch.tensor(float(tv_weight), dtype=torch.float32))            # as the kernel and vstab_loss_main_multi carry it
    loss = (per * torch.tensor(list(wts), dtype=torch.float64, device=pf.device)).sum() + tvw32 * s[:, T + 1].sum()
    return loss, grad, per


def loss_main_multi(flows: Dict[str, torch.Tensor], stab_image, unstab_image, objective: Objective, grads: Dict[str, torch.Tensor] = None):
    """loss_main of `objective` and (optionally) its flow gradients through ONE library call (`vstab_loss_main_multi`).  stab_image:
    [B,H,W,Ct] (24 channels in the scripts; any Ct that holds the objective's targets); flows / grads as in loss_main_fused.
    Returns (loss, per-target lossterms summed over the levels [T], unweighted), float64 CUDA tensors."""
    import ctypes as C
    stab, unstab = _f32c(stab_image, "stab_image"), _f32(unstab_image, "unstab_image", 3)
    B, H, W, Ct = stab.shape
    if unstab.shape[:3] != stab.shape[:3]:
        raise ValueError("stab_image / unstab_image must have the same batch and frame size")
    T, offs, wts, _w = _targets(objective.target_channels, objective.target_weights, Ct)
    desc = _level_descs(flows, grads, objective.tv_weights, B)
    L = _lib.lib()
    n = L.vstab_loss_main_multi_workspace_bytes(C.addressof(desc), len(LOSS_LEVELS), B, Ct, T)
    if n == 0:
        raise ValueError("loss_main_multi: the library rejects the level descriptors (1..8 levels, even channel counts >= 2, 8-byte aligned "
                         "flow / gradient buffers, level sizes below 2^31 / 3 pixels)")
    ws = torch.empty(n, dtype=torch.uint8, device=stab.device)
    out = torch.empty(1 + T, dtype=torch.float64, device=stab.device)
    with torch.cuda.device(stab.device):
        _lib.check(L.vstab_loss_main_multi(C.addressof(desc), len(LOSS_LEVELS), stab.data_ptr(), Ct, T, offs, wts, unstab.data_ptr(), B, H, W,
                                           out.data_ptr(), ws.data_ptr(), n, runtime.stream_ptr()))
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
    import ctypes as C
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
    L = _lib.lib()
    n = L.vstab_loss_report_workspace_bytes(C.addressof(desc), nl, B, Ct, T)
    if n == 0:
        raise ValueError("loss_report: the library rejects the level descriptors (even channel counts >= 2, 8-byte aligned flows, level "
                         "sizes below 2^31 / 3 pixels, B <= 65535)")
    ws = torch.empty(n, dtype=torch.uint8, device=stab.device)
    out = torch.empty(1 + T + 2 * nl, dtype=torch.float64, device=stab.device)
    with torch.cuda.device(stab.device):
        _lib.check(L.vstab_loss_report(C.addressof(desc), nl, stab.data_ptr(), Ct, T, offs, wts, unstab.data_ptr(), B, H, W,
                                       C.addressof(ptrs) if ptrs is not None else None, code, out.data_ptr(), ws.data_ptr(), n,
                                       runtime.stream_ptr()))
    return LossReport(out[0], out[1 + T:1 + T + nl], out[1 + T + nl:], out[1:1 + T], warped)


# ----------------------------------------------------------------------------- backward building blocks
def conv_wgrad(x, gout, k: int, stride: int, pad: int, cx_off: int = 0, cin: int = None, cg_off: int = 0, cout: int = None,
               dW=None, db=None, accumulate: bool = False, want_db: bool = True):
    """Filter and bias gradient of PadLayer(pad) -> Conv2d(k, stride, VALID) (model.py:807-844): what TF's autodiff
    returns for tf.nn.conv2d's filter, in the reference's HWIO layout.  x [B,Hi,Wi,Cs_x] (channels cx_off..+cin),
    gout [B,Ho,Wo,Cs_g] (channels cg_off..+cout).  Returns (dW [k,k,cin,cout], db [cout] or None)."""
    for t, name in ((x, "x"), (gout, "gout")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
            raise ValueError(f"{name} must be a float32 CUDA tensor [B,H,W,C]")
    x, gout = x.contiguous(), gout.contiguous()
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
    L = _lib.lib()
    nbytes = L.vstab_conv_wgrad_workspace_bytes(B, Ho, Wo, k, cin, cout)
    ws = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.vstab_conv_wgrad(x.data_ptr(), B, Hi, Wi, cs_x, cx_off, cin, gout.data_ptr(), Ho, Wo, cs_g, cg_off, cout,
                                      k, stride, pad, dW.data_ptr(), db.data_ptr() if want_db else None, 1 if accumulate else 0,
                                      ws.data_ptr(), ws.numel(), runtime.stream_ptr()))
    return dW, (db if want_db else None)


def conv_dgrad(gout, W, stride: int, pad: int, in_hw, cg_off: int = 0, cout: int = None, dx=None, cx_off: int = 0,
               accumulate: bool = False, bias=None):
    """Input gradient of PadLayer(pad) -> Conv2d(k, stride, VALID) with filter W [k,k,cin,cout] (CUDA tensor, HWIO):
    what TF's autodiff returns for tf.nn.conv2d's input.  gout [B,Ho,Wo,Cs_g] (channels cg_off..+cout); the result has
    the input's size in_hw and lands in channels cx_off..+cin of dx (allocated [B,Hi,Wi,cin] when None)."""
    if not torch.is_tensor(gout) or not gout.is_cuda or gout.dtype != torch.float32 or gout.dim() != 4:
        raise ValueError("gout must be a float32 CUDA tensor [B,Ho,Wo,C]")
    if not torch.is_tensor(W) or not W.is_cuda or W.dtype != torch.float32 or W.dim() != 4 or W.shape[0] != W.shape[1]:
        raise ValueError("W must be a float32 CUDA tensor [k,k,cin,cout]")
    gout, W = gout.contiguous(), W.contiguous()
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
    L = _lib.lib()
    nbytes = L.vstab_conv_dgrad_workspace_bytes(B, Ho, Wo, cs_g, cout, k, stride, pad, Hi, Wi, cs_x, cx_off, cin, 1 if accumulate else 0)
    if nbytes == 0:
        raise ValueError("conv_dgrad: unsupported geometry (stride 1 or 2, channel counts multiples of 4, matching sizes)")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=gout.device)
    with torch.cuda.device(gout.device):
        _lib.check(L.vstab_conv_dgrad(gout.data_ptr(), B, Ho, Wo, cs_g, cg_off, cout, W.data_ptr(),
                                      bias.data_ptr() if bias is not None else None, k, stride, pad, dx.data_ptr(),
                                      Hi, Wi, cs_x, cx_off, cin, 1 if accumulate else 0, ws.data_ptr(), ws.numel(),
                                      runtime.stream_ptr()))
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
    L = _lib.lib()
    sc = torch.empty(int(L.vstab_bn_scratch_bytes(rows, C)), dtype=torch.uint8, device=z.device)
    with torch.cuda.device(z.device):
        _lib.check(L.vstab_bn_lrelu_train_forward(z.data_ptr(), rows, cs, c_off, C, beta.data_ptr(),
                                                  moving_mean.data_ptr() if moving_mean is not None else None,
                                                  moving_var.data_ptr() if moving_var is not None else None, float(decay), float(eps),
                                                  mean.data_ptr(), rstd.data_ptr(), sc.data_ptr(), sc.numel(), runtime.stream_ptr()))
    return z, mean, rstd


def bn_lrelu_inference_forward(z, beta, moving_mean, moving_var, eps: float = 1e-5, c_off: int = 0, C: int = None):
    """BatchNormLayer(act=lrelu 0.1, is_train=False, gamma_init=None) IN PLACE on channels c_off..+C of z: y = lrelu((z - moving_mean)
    * rsqrt(moving_var + eps) + beta).  The moving statistics are read only.  Returns y (= z)."""
    rows, cs, C = _rows_view(z, c_off, C)
    with torch.cuda.device(z.device):
        _lib.check(_lib.lib().vstab_bn_lrelu_inference_forward(z.data_ptr(), rows, cs, c_off, C, beta.data_ptr(), moving_mean.data_ptr(),
                                                               moving_var.data_ptr(), float(eps), runtime.stream_ptr()))
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
    L = _lib.lib()
    sc = torch.empty(int(L.vstab_bn_scratch_bytes(rows, Cy)), dtype=torch.uint8, device=y.device)
    with torch.cuda.device(y.device):
        _lib.check(L.vstab_bn_lrelu_train_backward(y.data_ptr(), cs_y, cy_off, dy.data_ptr(), cs_g, cg_off, Cy, rows, beta.data_ptr(),
                                                   save_rstd.data_ptr(), dbeta.data_ptr(), 1 if accumulate else 0, sc.data_ptr(),
                                                   sc.numel(), runtime.stream_ptr()))
    return dy, dbeta


def lrelu_backward(y, dy, cy_off: int = 0, cg_off: int = 0, C: int = None):
    """dy *= (y > 0 ? 1 : 0.1) in place."""
    rows, cs_y, Cy = _rows_view(y, cy_off, C)
    _, cs_g, _ = _rows_view(dy, cg_off, C)
    with torch.cuda.device(y.device):
        _lib.check(_lib.lib().vstab_lrelu_backward(y.data_ptr(), cs_y, cy_off, dy.data_ptr(), cs_g, cg_off, Cy, rows, runtime.stream_ptr()))
    return dy


def resize_bilinear_backward(dout, in_hw, gain: float = 1.0, din=None):
    """din (+)= gain * adjoint of tf.image.resize_images(., dout's size) applied to dout [B,oh,ow,C]."""
    dout = dout.contiguous()
    B, oh, ow, C = dout.shape
    acc = din is not None
    if din is None:
        din = torch.empty((B, int(in_hw[0]), int(in_hw[1]), C), dtype=torch.float32, device=dout.device)
    with torch.cuda.device(dout.device):
        _lib.check(_lib.lib().vstab_resize_bilinear_backward(dout.data_ptr(), B, oh, ow, C, din.data_ptr(), din.shape[1], din.shape[2],
                                                             float(gain), 1 if acc else 0, runtime.stream_ptr()))
    return din


def _st_backward_args(src, dout, out_size, d_src, need_src, rank=4):
    """The checks every sampler backward makes of its input (rank 4: img [B,H,W,C], out_size (oh, ow); rank 5: vol [B,D,H,W,C],
    out_size (od, oh, ow)), of dout and of a given gradient to add into -> (src, dout, src's shape + out_size, d_src, accumulate)."""
    name, layout = ("img", "[B,H,W,C]") if rank == 4 else ("vol", "[B,D,H,W,C]")
    if not torch.is_tensor(src) or not src.is_cuda or src.dtype != torch.float32 or src.dim() != rank:
        raise ValueError(f"{name} must be a float32 CUDA tensor {layout}")
    src = src.contiguous()
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
    workspace, workspace_bytes, stream) -> (d_src or None, d_par or None).  entry and ws_query are the library's functions.  The
    parameter gradient [par_shape] and the workspace the library asks for (ws_query(*ws_args) bytes; never an empty allocation)
    exist only when need_par."""
    d_par, ws, n = None, None, 0
    if need_par:
        d_par = torch.empty(par_shape, dtype=torch.float32, device=dout.device)
        n = int(ws_query(*ws_args))
        ws = torch.empty(max(n, 8), dtype=torch.uint8, device=dout.device)
    with torch.cuda.device(dout.device):
        _lib.check(entry(*head, dout.data_ptr(), *out_size, d_src.data_ptr() if need_src else None, 1 if acc else 0,
                                     d_par.data_ptr() if need_par else None, ws.data_ptr() if need_par else None, n, runtime.stream_ptr()))
    return (d_src if need_src else None), d_par


def _st_interp(interp):
    if interp not in _lib.INTERP:
        raise ValueError("interp must be 'bilinear' or 'bicubic'")
    return _lib.INTERP[interp]


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
    L, head = _lib.lib(), (img.data_ptr(), B, H, W, C, theta.data_ptr(), tdim)
    entry, head = (L.vstab_st_transform_backward, head) if ip == 0 else (L.vstab_st_transform_interp_backward, (*head, ip))
    return _backward_with_param_grad(entry, head, dout, (oh, ow), d_img, acc, need_img, need_theta, (B, tdim),
                                     L.vstab_st_transform_backward_workspace_bytes, (B, H, W, C, oh, ow))


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
    L, head = _lib.lib(), (img.data_ptr(), B, H, W, C, theta.data_ptr(), kind)
    entry, head = (L.vstab_st_symmetry_transform_backward, head) if ip == 0 else (L.vstab_st_symmetry_transform_interp_backward, (*head, ip))
    return _backward_with_param_grad(entry, head, dout, (oh, ow), d_img, acc, need_img, need_theta, (B, tdim),
                                     L.vstab_st_symmetry_transform_backward_workspace_bytes, (B, H, W, C, oh, ow))


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
    L = _lib.lib()
    if ref is None:
        entry, head = L.vstab_homography_warp_backward, (img.data_ptr(), B, H, W, C, M.data_ptr())
    else:
        if not torch.is_tensor(ref) or ref.device != img.device or ref.dtype != torch.float32 or ref.numel() != 9:
            raise ValueError("ref must be a float32 tensor of 9 elements beside img")
        ref = ref.contiguous()
        entry, head = L.vstab_transform_image_backward, (img.data_ptr(), B, H, W, C, ref.data_ptr(), M.data_ptr())
    return _backward_with_param_grad(entry, head, dout, (oh, ow), d_img, acc, need_img, need_M, (B, 3, 3),
                                     L.vstab_homography_warp_backward_workspace_bytes, (B, H, W, C, oh, ow))


def vec2mtrx_backward(p, d_out, warp_type, warp_approx):
    """Gradient of warp.vec2mtrx: p [B,8] (warp_type 'homography') or [B,6] ('affine'), d_out [B,3,3] the gradient of the matrix ->
    d p of p's shape.  In double from the fp32 p, rounded once; bit-reproducible."""
    dim = {"homography": 8, "affine": 6}.get(warp_type)
    if dim is None:
        raise ValueError("warp_type must be 'homography' or 'affine'")
    if not torch.is_tensor(p) or not p.is_cuda or p.dtype != torch.float32 or p.dim() != 2 or p.shape[1] != dim:
        raise ValueError(f"p must be a float32 CUDA tensor [B,{dim}]")
    B = p.shape[0]
    if not torch.is_tensor(d_out) or d_out.device != p.device or d_out.dtype != torch.float32 or d_out.numel() != 9 * B:
        raise ValueError("d_out must be a float32 tensor [B,3,3] beside p")
    p, d_out = p.contiguous(), d_out.contiguous()
    d_p = torch.empty_like(p)
    with torch.cuda.device(p.device):
        _lib.check(_lib.lib().vstab_vec2mtrx_backward(p.data_ptr(), B, dim, int(warp_approx), d_out.data_ptr(), d_p.data_ptr(),
                                                      runtime.stream_ptr()))
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
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().vstab_warp_flow_backward(img.data_ptr(), flow.data_ptr(), dout.data_ptr(), B, H, W, C,
                                                       d_img.data_ptr() if need_img else None, d_flow.data_ptr() if need_flow else None,
                                                       1 if acc else 0, runtime.stream_ptr()))
    return (d_img if need_img else None), d_flow


def get_pixel_value_backward(dout, x, y, img_hw, d_img=None):
    """Gradient of warp_flow.get_pixel_value with respect to its image: dout [B,H,W,C] scattered into d img [B,Hi,Wi,C] (img_hw =
    (Hi, Wi)) at the forward's clipped indices x, y (int32 [B,H,W]).  A given d_img is added into.  Float atomics: where several
    indices meet, the last bits depend on the arrival order."""
    if not torch.is_tensor(dout) or not dout.is_cuda or dout.dtype != torch.float32 or dout.dim() != 4:
        raise ValueError("dout must be a float32 CUDA tensor [B,H,W,C]")
    dout = dout.contiguous()
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
    with torch.cuda.device(dout.device):
        _lib.check(_lib.lib().vstab_get_pixel_value_backward(dout.data_ptr(), x.data_ptr(), y.data_ptr(), d_img.data_ptr(), B, H, W, C, Hi, Wi,
                                                             1 if acc else 0, runtime.stream_ptr()))
    return d_img


def flow_resize_scale_backward(dout, in_hw, net_h: int, net_w: int):
    """Gradient of warp_flow.flow_to_output_res with respect to predict_flow2 [B,h,w,2] (in_hw = (h, w)) for the gradient dout
    [B,oh,ow,2] of the output-resolution flow: (net_h / h) * resize^T(dout * (ow / net_w, oh / net_h)), one gain per channel.  A
    gather in a fixed order: bit-reproducible."""
    if not torch.is_tensor(dout) or not dout.is_cuda or dout.dtype != torch.float32 or dout.dim() != 4 or dout.shape[3] != 2:
        raise ValueError("dout must be a float32 CUDA tensor [B,oh,ow,2]")
    dout = dout.contiguous()
    B, oh, ow, _ = dout.shape
    h, w = int(in_hw[0]), int(in_hw[1])
    d_flow = torch.empty((B, h, w, 2), dtype=torch.float32, device=dout.device)
    with torch.cuda.device(dout.device):
        _lib.check(_lib.lib().vstab_flow_resize_scale_backward(dout.data_ptr(), B, oh, ow, d_flow.data_ptr(), h, w, int(net_h), int(net_w),
                                                               runtime.stream_ptr()))
    return d_flow


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
    L, head = _lib.lib(), (img.data_ptr(), B, H, W, C, theta.data_ptr(), g, linv_t.data_ptr())
    entry, head = (L.vstab_st_elastic_transform_backward, head) if ip == 0 else (L.vstab_st_elastic_transform_interp_backward, (*head, ip))
    return _backward_with_param_grad(entry, head, dout, (oh, ow), d_img, acc, need_img, need_theta, (B, 2 * K),
                                     L.vstab_st_elastic_transform_backward_workspace_bytes, (B, H, W, C, g, oh, ow))


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
    with torch.cuda.device(img.device):
        _lib.check(getattr(_lib.lib(), entry)(img.data_ptr(), B, H, W, C, x.data_ptr(), y.data_ptr(), dout.data_ptr(), oh, ow,
                                              d_img.data_ptr() if need_img else None, 1 if acc else 0,
                                              d_x.data_ptr() if need_x else None, d_y.data_ptr() if need_y else None, runtime.stream_ptr()))
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
    L = _lib.lib()
    return _backward_with_param_grad(L.vstab_st3d_transform_backward, (vol.data_ptr(), B, D, H, W, C, theta.data_ptr()), dout, (od, oh, ow),
                                     d_vol, acc, need_vol, need_theta, (B, 12), L.vstab_st3d_transform_backward_workspace_bytes,
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
    ptr = lambda t: t.data_ptr() if t is not None else None          # noqa: E731
    with torch.cuda.device(vol.device):
        _lib.check(_lib.lib().vstab_st3d_bilinear_interp_backward(vol.data_ptr(), B, D, H, W, C, x.data_ptr(), y.data_ptr(), z.data_ptr(), od, oh,
                                                                  ow, int(edge_size), dout.data_ptr(), d_vol.data_ptr() if need_vol else None,
                                                                  1 if acc else 0, ptr(d_x), ptr(d_y), ptr(d_z), runtime.stream_ptr()))
    return (d_vol if need_vol else None), d_x, d_y, d_z


def pad_nearest_upsample(src, H: int, W: int):
    """PadLayer(1) -> nearest resize (align_corners=True) to HxW (model.py:795-802, 882-884); C % 4 == 0."""
    src = src.contiguous()
    B, h2, w2, C = src.shape
    out = torch.empty((B, H, W, C), dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        _lib.check(_lib.lib().vstab_pad_nearest_upsample(src.data_ptr(), B, h2, w2, C, out.data_ptr(), H, W, runtime.stream_ptr()))
    return out


def pad_nearest_upsample_backward(dout, src_hw, dsrc=None):
    dout = dout.contiguous()
    B, H, W, C = dout.shape
    acc = dsrc is not None
    if dsrc is None:
        dsrc = torch.empty((B, int(src_hw[0]), int(src_hw[1]), C), dtype=torch.float32, device=dout.device)
    with torch.cuda.device(dout.device):
        _lib.check(_lib.lib().vstab_pad_nearest_upsample_backward(dout.data_ptr(), B, H, W, C, dsrc.data_ptr(), dsrc.shape[1], dsrc.shape[2],
                                                                  1 if acc else 0, runtime.stream_ptr()))
    return dsrc


def conv3x3_winograd(x, W, transpose: bool = False, bias=None, y=None, cx_off: int = 0, cy_off: int = 0, act: int = 0):
    """3x3 stride-1 pad-1 convolution (transpose=False: x [..,cin] -> [..,cout]) or its input gradient (transpose=True:
    x = output gradient [..,cout] -> dx [..,cin]) in Winograd F(2x2,3x3) form; W [3,3,cin,cout] CUDA tensor.  act 0 none,
    1 leaky relu 0.1, 3 add to what is in y."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.float32 or x.dim() != 4:
        raise ValueError("x must be a float32 CUDA tensor [B,H,W,C]")
    x, W = x.contiguous(), W.contiguous()
    B, H, Wd, cs_x = x.shape
    cin, cout = int(W.shape[2]), int(W.shape[3])
    n_out = cin if transpose else cout
    if y is None:
        y = torch.empty((B, H, Wd, n_out), dtype=torch.float32, device=x.device)
        cy_off = 0
    L = _lib.lib()
    nbytes = L.vstab_conv3x3_winograd_workspace_bytes(B, H, Wd, cin, cout, 1 if transpose else 0)
    if nbytes == 0:
        raise ValueError("conv3x3_winograd: unsupported geometry (reduction channels % 32, output channels % 64, < 2 GiB per tensor)")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.vstab_conv3x3_winograd(x.data_ptr(), B, H, Wd, cs_x, cx_off, W.data_ptr(), cin, cout, 1 if transpose else 0,
                                            bias.data_ptr() if bias is not None else None, y.data_ptr(), y.shape[3], cy_off, act,
                                            ws.data_ptr(), ws.numel(), runtime.stream_ptr()))
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
    L = _lib.lib()
    n = L.vstab_conv3x3_winograd_wgrad_workspace_bytes(B, H, W, cin, cout)
    if n == 0:
        raise ValueError("conv3x3_winograd_wgrad: channel counts must be multiples of 4 (and tensors < 2 GiB)")
    if dW is None:
        dW = torch.empty((3, 3, cin, cout), dtype=torch.float32, device=x.device)
    ws = torch.empty(n, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(L.vstab_conv3x3_winograd_wgrad(x.data_ptr(), B, H, W, cs_x, cx_off, cin, gout.data_ptr(), cs_g, cg_off, cout,
                                                  dW.data_ptr(), ws.data_ptr(), n, runtime.stream_ptr()))
    return dW


def ssim_backward(img1, img2, dout, size: int = 9, sigma: float = 0.5, need_img1: bool = True, need_img2: bool = True):
    """Gradients of utils.tf_ssim's value s (utils.py:111; l**0 and c**0 are constants) with respect to both images [B,H,W,1]: (d img1
    or None, d img2 or None).  dout is the gradient of the map, [B,H-size+1,W-size+1,1], or -- one dimension, [B] -- that of the
    per-sample means, broadcast over the sample's map inside the kernel.  need_img1 / need_img2 False skips that image.  Gathered
    through the flipped window without atomics: bit-reproducible, and what utils' autograd functions call."""
    for t, name in ((img1, "img1"), (img2, "img2")):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or t.shape[3] != 1:
            raise ValueError(f"{name} must be a float32 CUDA tensor [B,H,W,1]")
    if img1.shape != img2.shape or img1.device != img2.device:
        raise ValueError("img1 and img2 must have the same shape and device")
    if not need_img1 and not need_img2:
        return None, None
    a, b, size = img1.contiguous(), img2.contiguous(), int(size)
    B, H, W, _ = a.shape
    L = _lib.lib()
    n = int(L.vstab_ssim_backward_workspace_bytes(B, H, W, size))
    if n == 0:
        raise ValueError(f"ssim_backward: need B >= 1, 1 <= size <= 11 and images of at least size x size, got {B}x{H}x{W}, size {size}")
    per_sample = torch.is_tensor(dout) and dout.dim() == 1
    want = B if per_sample else B * (H - size + 1) * (W - size + 1)
    if not torch.is_tensor(dout) or dout.device != a.device or dout.dtype != torch.float32 or dout.numel() != want:
        raise ValueError(f"dout must be a float32 tensor of {want} elements beside the images")
    dout = dout.contiguous()
    d1 = torch.empty_like(a) if need_img1 else None
    d2 = torch.empty_like(a) if need_img2 else None
    ws = torch.empty(n, dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        _lib.check(L.vstab_ssim_backward(a.data_ptr(), b.data_ptr(), B, H, W, size, float(sigma), None if per_sample else dout.data_ptr(),
                                         dout.data_ptr() if per_sample else None, d1.data_ptr() if need_img1 else None,
                                         d2.data_ptr() if need_img2 else None, ws.data_ptr(), n, runtime.stream_ptr()))
    return d1, d2


# ----------------------------------------------------------------------------- recurrent cells (cell.py): gate-stage backward
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
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4 or (shape is not None and tuple(t.shape) != tuple(shape)):
        raise ValueError(f"{name} must be a float32 CUDA tensor {list(shape) if shape is not None else '[B,H,W,F]'}")
    return t.contiguous()


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


def _ptr(t):
    return t.data_ptr() if t is not None else None


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
    L = _lib.lib()
    n = int(L.vstab_convlstm_gates_backward_workspace_bytes(B, H, W, F, int(normalize), int(peephole)))
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=c.device)
    pe = [p.contiguous() for p in peepholes] if peephole else [None] * 3
    with torch.cuda.device(c.device):
        _lib.check(L.vstab_convlstm_gates_backward(
            y.data_ptr(), y.shape[3], c.data_ptr(), _ptr(pe[0]), _ptr(pe[1]), _ptr(pe[2]), _ptr(gamma), _ptr(beta),
            _ptr(stats[0]) if normalize else None, _ptr(stats[1]) if normalize else None, dhp, dhs, _ptr(dcn), B, H, W, F, float(forget_bias),
            int(act), int(normalize), int(peephole), dy.data_ptr(), dy.shape[3], dc.data_ptr(), _ptr(g["W_ci"]), _ptr(g["W_cf"]), _ptr(g["W_co"]),
            _ptr(g["gamma"]), _ptr(g["beta"]), 1 if accumulate else 0, ws.data_ptr(), ws.numel(), runtime.stream_ptr()))
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
    L = _lib.lib()
    n = int(L.vstab_convgru_backward_workspace_bytes(B, H, W, F, int(normalize)))
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=u.device)
    with torch.cuda.device(u.device):
        _lib.check(L.vstab_convgru_update_backward(y2.data_ptr(), y2.shape[3], hp, hs, u.data_ptr(), _ptr(gamma), _ptr(beta), _ptr(stats), dnp, dns, B, H,
                                                   W, F, int(act), int(normalize), dy2.data_ptr(), dy2.shape[3], du.data_ptr(), dhp, dhs,
                                                   _ptr(g["gamma"]), _ptr(g["beta"]), 1 if accumulate else 0, ws.data_ptr(), ws.numel(),
                                                   runtime.stream_ptr()))
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
    L = _lib.lib()
    n = int(L.vstab_convgru_backward_workspace_bytes(B, H, W, F, int(normalize)))
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device=du.device)
    with torch.cuda.device(du.device):
        _lib.check(L.vstab_convgru_gates_backward(y.data_ptr(), y.shape[3], hp, hs, _ptr(gamma), _ptr(beta), _ptr(stats), du.data_ptr(), rp, rs, B, H, W, F,
                                                  int(normalize), dy.data_ptr(), dy.shape[3], dhp, dhs, _ptr(g["gamma"]), _ptr(g["beta"]),
                                                  1 if accumulate else 0, ws.data_ptr(), ws.numel(), runtime.stream_ptr()))
    return dy, g
