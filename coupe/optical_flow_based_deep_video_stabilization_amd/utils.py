"""Drop-ins for the image-similarity measures of the reference's `utils.py`: `_tf_fspecial_gauss` (:74-89), `tf_ssim` (:91-124) and
`tf_ms_ssim` (:126-166), as metrics and as differentiable loss terms.  Images are float32 CUDA tensors [B,H,W,1]; the arithmetic runs
in HIP kernels (csrc/ssim_ops.hip, C ABI in include/vstab.h) and there is no CPU path.

What the reference computes is not the textbook SSIM: the luminance and contrast terms enter as `l**0` and `c**0` (:113), so the value
is the squared structure term  s = (s12^2 + C3) / (s1 s2 + C3),  C3 = 0.03^2 / 2  (:111) over VALID windows of
`_tf_fspecial_gauss(size, sigma)`, whose default sigma of 0.5 leaves all but about 1e-3 of the weight in the central 3x3.  One
channel only: the reference's conv2d with a [k,k,1,1] window takes nothing else.  The kernels apply the window in its separable
form (it is an outer product), so results differ from a 2-D correlation in the last bits.

Two things are kept or changed on purpose:
  * `tf_ms_ssim` keeps the reference's reduction as written (:162): `reduce_prod` has no axis, so the [batch_size] result holds the
    SAME number in every entry, the product of all level x batch_size per-sample means (times `ml[level-1]`, which is 1).
  * Gradients (torch.autograd, with respect to both images) treat `l**0` and `c**0` as the constant 1.  TensorFlow's gradient of
    pow(c, 0) is 0 * c^-1, which is NaN wherever a window is flat (sqrt(0)) or fp32 cancellation leaves a variance slightly
    negative; here the gradient is that of s alone and is finite there.
The autograd path is taken only when gradients are enabled and an image requires grad.  Values and gradients are summed without
atomics in a fixed order: two runs give the same bits.

`fix_image_tf` (:434), the image log's float -> uint8 conversion, is here too."""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import runtime
from ._autograd import wants_grad as _wants_grad
from .runtime import ptr as _ptr

_MAX_SIZE = 11


def _tf_fspecial_gauss(size, sigma):
    """The normalised Gaussian window [size,size,1,1] (float32, host) of utils.py:74-89: offsets -size//2+1 .. size//2 with floor
    division, so size 9 covers -4..4 and size 8 covers -3..4."""
    size = int(size)
    if size < 1:
        raise ValueError("size must be >= 1")
    c = torch.arange(-size // 2 + 1, size // 2 + 1, dtype=torch.float32)
    xx, yy = c.reshape(size, 1), c.reshape(1, size)
    g = torch.exp(-((xx ** 2 + yy ** 2) / (2.0 * float(sigma) ** 2)))
    return (g / g.sum()).reshape(size, size, 1, 1)


def _image(t, name):
    t = runtime.f32_cuda(t, name, 4, layout="[B,H,W,1]")
    if t.shape[3] != 1:
        raise ValueError(f"{name} has {t.shape[3]} channels: the reference's [k,k,1,1] window takes one channel only")
    return t


def _pair(img1, img2, size, sigma):
    a, b = _image(img1, "img1"), _image(img2, "img2")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError("img1 and img2 must have the same shape and device")
    size = int(size)
    if not 1 <= size <= _MAX_SIZE:
        raise ValueError(f"size must be 1..{_MAX_SIZE}")
    if not float(sigma) > 0.0:
        raise ValueError("sigma must be positive")
    if a.shape[0] < 1 or a.shape[1] < size or a.shape[2] < size:
        raise ValueError(f"images of {a.shape[1]}x{a.shape[2]} are smaller than the {size}x{size} window")
    return a, b, size, float(sigma)


def _ssim_call(a, b, size, sigma, want_map, want_means):
    B, H, W, _ = a.shape
    smap = torch.empty((B, H - size + 1, W - size + 1, 1), dtype=torch.float32, device=a.device) if want_map else None
    means, ws = None, None
    if want_means:
        means = torch.empty((B,), dtype=torch.float32, device=a.device)
        ws = runtime.workspace(a.device, "vstab_ssim_forward_workspace_bytes", B, H, W, size)
    runtime.call(a.device, "vstab_ssim_forward", a.data_ptr(), b.data_ptr(), B, H, W, size, sigma, _ptr(smap), _ptr(means), _ptr(ws),
                 ws.numel() if want_means else 0)
    return smap, means


def ssim_backward(img1, img2, dout, size: int = 9, sigma: float = 0.5, need_img1: bool = True, need_img2: bool = True):
    """Gradients of tf_ssim's value s (utils.py:111; l**0 and c**0 are constants) with respect to both images [B,H,W,1]: (d img1
    or None, d img2 or None).  dout is the gradient of the map, [B,H-size+1,W-size+1,1], or -- one dimension, [B] -- that of the
    per-sample means, broadcast over the sample's map inside the kernel.  need_img1 / need_img2 False skips that image.  Gathered
    through the flipped window without atomics: bit-reproducible, and what the autograd functions below call."""
    a, b = (runtime.f32_cuda(t, name, 4, 1, "[B,H,W,1]") for t, name in ((img1, "img1"), (img2, "img2")))
    if img1.shape != img2.shape or img1.device != img2.device:
        raise ValueError("img1 and img2 must have the same shape and device")
    if not need_img1 and not need_img2:
        return None, None
    size = int(size)
    B, H, W, _ = a.shape
    ws = runtime.workspace(a.device, "vstab_ssim_backward_workspace_bytes", B, H, W, size, refused=(
        f"ssim_backward: need B >= 1, 1 <= size <= 11 and images of at least size x size, got {B}x{H}x{W}, size {size}"))
    per_sample = torch.is_tensor(dout) and dout.dim() == 1
    want = B if per_sample else B * (H - size + 1) * (W - size + 1)
    if not torch.is_tensor(dout) or dout.device != a.device or dout.dtype != torch.float32 or dout.numel() != want:
        raise ValueError(f"dout must be a float32 tensor of {want} elements beside the images")
    dout = dout.contiguous()
    d1 = torch.empty_like(a) if need_img1 else None
    d2 = torch.empty_like(a) if need_img2 else None
    runtime.call(a.device, "vstab_ssim_backward", a.data_ptr(), b.data_ptr(), B, H, W, size, float(sigma), None if per_sample else dout.data_ptr(),
                 dout.data_ptr() if per_sample else None, _ptr(d1), _ptr(d2), ws.data_ptr(), ws.numel())
    return d1, d2


class _SsimMapFn(torch.autograd.Function):
    """s map [B,oh,ow,1] with its HIP backward (ssim_backward)."""

    @staticmethod
    def forward(ctx, a, b, size, sigma):
        ctx.save_for_backward(a, b)
        ctx.size, ctx.sigma = size, sigma
        return _ssim_call(a, b, size, sigma, True, False)[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        a, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        d1, d2 = ssim_backward(a, b, dout, ctx.size, ctx.sigma, need_img1=need[0], need_img2=need[1])
        return d1, d2, None, None


class _SsimMeansFn(torch.autograd.Function):
    """per-sample means [B] of the s map (no map is stored) with the same backward; the upstream scalar of a sample is broadcast
    inside the kernel."""

    @staticmethod
    def forward(ctx, a, b, size, sigma):
        ctx.save_for_backward(a, b)
        ctx.size, ctx.sigma = size, sigma
        return _ssim_call(a, b, size, sigma, False, True)[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, dmeans):
        a, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        d1, d2 = ssim_backward(a, b, dmeans.reshape(-1), ctx.size, ctx.sigma, need_img1=need[0], need_img2=need[1])
        return d1, d2, None, None


def _ssim_map(a, b, size, sigma):
    if _wants_grad(a, b):
        return _SsimMapFn.apply(a, b, size, sigma)
    return _ssim_call(a, b, size, sigma, True, False)[0]


def _ssim_means(a, b, size, sigma):
    if _wants_grad(a, b):
        return _SsimMeansFn.apply(a, b, size, sigma)
    return _ssim_call(a, b, size, sigma, False, True)[1]


def _avg_pool_call(x):
    B, H, W, C = x.shape
    out = torch.empty((B, (H + 1) // 2, (W + 1) // 2, C), dtype=torch.float32, device=x.device)
    runtime.call(x.device, "vstab_avgpool2x2_same", x.data_ptr(), B, H, W, C, out.data_ptr())
    return out


class _AvgPoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.in_shape = tuple(x.shape)
        return _avg_pool_call(x)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        B, H, W, C = ctx.in_shape
        dout = dout.contiguous()
        dx = torch.empty(ctx.in_shape, dtype=torch.float32, device=dout.device)
        runtime.call(dout.device, "vstab_avgpool2x2_same_backward", dout.data_ptr(), B, H, W, C, dx.data_ptr())
        return dx


def avg_pool_2x2_same(x):
    """tf.nn.avg_pool(x, [1,2,2,1], [1,2,2,1], padding='SAME') on a float32 CUDA tensor [B,H,W,C] (utils.py:146-147): the output is
    [B,ceil(H/2),ceil(W/2),C] and a window that hangs over the edge averages the pixels that exist.  Differentiable."""
    x = runtime.f32_cuda(x, "x", 4, layout="[B,H,W,C]")
    return _AvgPoolFn.apply(x) if _wants_grad(x) else _avg_pool_call(x)


def tf_ssim(img1, img2, mean_metric=True, cs_map=False, size=9, sigma=0.5):
    """utils.py:91-124 on float32 CUDA images [B,H,W,1]: s = (s12^2 + C3) / (s1 s2 + C3) over VALID size x size Gaussian windows, a
    map [B,H-size+1,W-size+1,1].  cs_map=True returns the pair (l**0, c**0 * s) = (ones, s) (:113); mean_metric takes the mean over
    all elements (of each member of the pair).  The mean forms store no map.  Differentiable with respect to both images, with
    l**0 and c**0 as constants (module docstring).  size 1..11."""
    a, b, size, sigma = _pair(img1, img2, size, sigma)
    if mean_metric:
        value = _ssim_means(a, b, size, sigma).mean()
        return (torch.ones_like(value), value) if cs_map else value
    smap = _ssim_map(a, b, size, sigma)
    return (torch.ones_like(smap), smap) if cs_map else smap


def tf_ms_ssim(img1, img2, batch_size, mean_metric=True, level=5):
    """utils.py:126-166: per level the per-sample mean of tf_ssim's cs map (size 9, sigma 0.5), then both images halved by the 2x2
    SAME average pool; all level weights are 1.  The reduction is the reference's as written (:162): `reduce_prod` has no axis, so
    the result is a [batch_size] vector whose EVERY entry is the product of all level x batch_size per-sample means (times
    ml[level-1] = 1) -- the samples are not scored separately.  mean_metric takes the mean of that vector, i.e. the same number.
    batch_size must be the images' B; every level's image must hold a 9x9 window (5 levels: H, W >= 129).  Differentiable; the
    gradients of all levels accumulate into the full-size images through the pool's adjoint."""
    a, b, size, sigma = _pair(img1, img2, 9, 0.5)
    level = int(level)
    if level < 1:
        raise ValueError("level must be >= 1")
    if int(batch_size) != a.shape[0]:
        raise ValueError(f"batch_size {batch_size} is not the images' batch {a.shape[0]}")
    h, w = a.shape[1], a.shape[2]
    for lv in range(level):
        if h < size or w < size:
            raise ValueError(f"level {lv} would be {h}x{w}, smaller than the {size}x{size} window")
        h, w = (h + 1) // 2, (w + 1) // 2
    mcs = []
    for lv in range(level):
        mcs.append(_ssim_means(a, b, size, sigma))
        if lv + 1 < level:                       # the reference also pools after the last level; nothing reads that result
            a, b = avg_pool_2x2_same(a), avg_pool_2x2_same(b)
    value = torch.prod(torch.stack(mcs, dim=0)).expand(int(batch_size))
    return value.mean() if mean_metric else value


def fix_image_tf(image, norm_value):
    """utils.py:434: tf.cast(image / norm_value * 255., tf.uint8) on a float tensor, for the image log (main:365-371).  The quotient
    and the product are rounded in the image's type, the result is saturated to 0..255 and then truncated toward zero: TensorFlow's
    cast is undefined outside the range, and a warped frame holds tiny negative values where clamped corners make the bilinear
    weights cancel.  The same rule as the uint8 previews of `training.loss_report` (norm_value 1).  Plain torch, no kernel."""
    if not torch.is_tensor(image) or not image.is_floating_point():
        raise ValueError("image must be a float tensor")
    return (image / norm_value * 255.0).clamp(0.0, 255.0).to(torch.uint8)
