"""Drop-ins for the reference's `warp.py` (named by BASELINE.json's north_star; dead code in the
reference: only `import warp` at config.py:3, and `config.py` never defines the `warpType`,
`refMtrx`, `warpApprox`, `batch_size`, `height`, `width` fields these functions read).  `config` is
any object carrying those attributes; images and parameters are float32 CUDA tensors.  The
arithmetic runs in HIP kernels (csrc/sampler_ops.hip); `fit` is host numpy like the original.

Differentiable (torch.autograd, HIP backward kernels): `vec2mtrx` with respect to `p`; `warpImage` with respect to the image and `M`;
`transformImage` and `transformCropImage` with respect to the image and `pMtrx` (`refMtrx` is configuration and gets no gradient);
`compose` and `inverse` are torch arithmetic.  floor, ceil and the int casts have zero derivative, so where a source coordinate is an
exact integer that axis' slope is 0, as in the reference.  The image gradient is summed by float atomics (last bits may differ between
runs); those of `M`, `pMtrx` and `p` are bit-reproducible.  The autograd path is taken only when gradients are enabled and an input
requires grad; otherwise the calls are the forward launches alone and the results carry no `grad_fn`."""
from __future__ import annotations

import numpy as np
import torch

from . import _autograd, runtime, sampler_grad


def fit(Xsrc, Xdst):
    """Least-squares affine map Xsrc -> Xdst ([N,2] point sets) as a 3x3 float32 matrix (warp.py:6-14)."""
    Xsrc = np.asarray(Xsrc, dtype=np.float64)
    Xdst = np.asarray(Xdst, dtype=np.float64)
    n = len(Xsrc)
    A = np.zeros((2 * n, 6))
    A[:n, 0:2], A[:n, 2] = Xsrc, 1.0
    A[n:, 3:5], A[n:, 5] = Xsrc, 1.0
    b = np.concatenate([Xdst[:, 0], Xdst[:, 1]])
    sol = np.linalg.lstsq(A, b, rcond=None)[0]
    return np.array([[sol[0], sol[1], sol[2]], [sol[3], sol[4], sol[5]], [0, 0, 1]], dtype=np.float32)


def compose(config, p, dp):
    return p + dp


def inverse(config, p):
    return -p


def _f32_cuda(t, name):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t, dtype=np.float32))
    if not t.is_cuda:
        runtime._require_gpu()
        t = t.cuda()
    return t.to(torch.float32).contiguous()


def _vec2mtrx_call(p, warp_type, dim, approx):
    B = p.shape[0]
    out = torch.empty((B, 3, 3), dtype=torch.float32, device=p.device)
    runtime.call(p.device, "vstab_vec2mtrx", p.data_ptr(), B, dim, approx, out.data_ptr())
    return out


def _vec2mtrx_backward(saved, d_out, needs, statics):
    warp_type, _, approx = statics
    return (sampler_grad.vec2mtrx_backward(saved[0], d_out, warp_type, approx),)


def vec2mtrx(config, p):
    """p [B,8] (homography: sl(3) generator, warp.py:28-30) or [B,6] (affine, :31-34) -> [B,3,3]
    Taylor matrix exponential with config.warpApprox terms (:37-42).  Differentiable with respect to p."""
    p = _f32_cuda(p, "p")
    if config.warpType == "homography":
        dim = 8
    elif config.warpType == "affine":
        dim = 6
    else:
        raise AssertionError("warpType must be 'homography' or 'affine'")
    if p.shape[1] != dim:
        raise ValueError(f"p must be [B,{dim}] for warpType={config.warpType}")
    return _autograd.apply(_vec2mtrx_call, _vec2mtrx_backward, (p,), (config.warpType, dim, int(config.warpApprox)))


def _warp_call(image, mat, ref, oh, ow):
    """ref None: mat [B,9] is M = refMtrx . pMtrx; otherwise mat is pMtrx and refMtrx . pMtrx (warp.py:48-49, 91-92: a tf.matmul in the
    reference) is composed inside the warp launch -- every product and sum rounded to fp32 -- not by a library GEMM in front of it."""
    B, Hi, Wi, Cc = image.shape
    out = torch.empty((B, oh, ow, Cc), dtype=torch.float32, device=image.device)
    if ref is None:
        runtime.call(image.device, "vstab_homography_warp", image.data_ptr(), B, Hi, Wi, Cc, mat.data_ptr(), out.data_ptr(), oh, ow)
    else:
        runtime.call(image.device, "vstab_transform_image", image.data_ptr(), B, Hi, Wi, Cc, ref.data_ptr(), mat.data_ptr(), out.data_ptr(), oh, ow)
    return out


def _warp_backward(saved, dout, needs, statics):
    """d image and d M, or with ref d pMtrx."""
    image, mat = saved
    ref, oh, ow = statics
    d_img, d_mat = sampler_grad.homography_warp_backward(image, mat, dout, (oh, ow), need_img=needs[0], need_M=needs[1], ref=ref)
    return d_img, (d_mat.reshape(mat.shape) if d_mat is not None else None)


def _warp(image, mat, ref, oh, ow):
    return _autograd.apply(_warp_call, _warp_backward, (image, mat), (ref, oh, ow))


def warpImage(image, M, oh, ow):
    """The warp of transformImage given the composed matrices M = refMtrx . pMtrx [B,3,3] (not a reference symbol: the reference
    composes inside transformImage, as `transformImage` below does inside its launch).  Differentiable with respect to image and M."""
    image = _f32_cuda(image, "image")
    M = _f32_cuda(M, "matrix").reshape(image.shape[0], 9)
    return _warp(image, M, None, oh, ow)


def _warp_ref(image, ref, pMtrx, oh, ow):
    image = _f32_cuda(image, "image")
    pM = _f32_cuda(pMtrx, "pMtrx").to(image.device).reshape(image.shape[0], 9)
    ref = _f32_cuda(ref, "refMtrx").to(image.device).reshape(9).detach()          # configuration: no gradient
    return _warp(image, pM, ref, oh, ow)


def transformImage(config, image, pMtrx):
    """image [B,H,W,3] warped by refMtrx . pMtrx on the canonical [-1,1]^2 grid (warp.py:46-86).  Differentiable with respect to image
    and pMtrx; refMtrx is configuration."""
    return _warp_ref(image, config.refMtrx, pMtrx, int(config.height), int(config.width))


def transformCropImage(config, image, pMtrx):
    """As transformImage with refMtrx_b, source [B,dataH,dataW,3], output height x W (warp.py:89-129)."""
    return _warp_ref(image, config.refMtrx_b, pMtrx, int(config.height), int(config.W))
