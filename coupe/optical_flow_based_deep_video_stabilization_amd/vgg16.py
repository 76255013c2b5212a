"""Drop-in for the reference's `vgg16.py` (Vgg16.build, vgg16.py:25-64): the 13-conv / 5-pool VGG16
trunk, BASELINE.json config 5.  `vgg16.npy` is not shipped with the reference and cannot be fetched
offline, so besides a path the constructor accepts the dict itself ({layer: [W (3,3,Cin,Cout), b]},
the structure `np.load(...).item()` yields, vgg16.py:22) or a seed for synthetic weights.
All arithmetic runs in libvstab_hip.so (implicit-GEMM MFMA conv + ReLU epilogue, max-pool kernel).
The trunk is differentiable: `Vgg16.backward` pulls gradients at any of the 18 outputs back to the input and
the filters, `Vgg16.features` is the autograd entry on top of it, `preprocess` carries its factor of 255."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from torch.autograd.function import once_differentiable

from . import _autograd, _lib, nldf_loss, runtime

VGG_MEAN = [103.939, 116.779, 123.68]     # vgg16.py:7 (BGR order; NLDF.py:29 applies it to RGB as is)

LAYERS = (("conv1_1", 3, 64), ("conv1_2", 64, 64), ("conv2_1", 64, 128), ("conv2_2", 128, 128),
          ("conv3_1", 128, 256), ("conv3_2", 256, 256), ("conv3_3", 256, 256), ("conv4_1", 256, 512),
          ("conv4_2", 512, 512), ("conv4_3", 512, 512), ("conv5_1", 512, 512), ("conv5_2", 512, 512),
          ("conv5_3", 512, 512))
OUTPUTS = ("conv1_1", "conv1_2", "pool1", "conv2_1", "conv2_2", "pool2", "conv3_1", "conv3_2", "conv3_3", "pool3",
           "conv4_1", "conv4_2", "conv4_3", "pool4", "conv5_1", "conv5_2", "conv5_3", "pool5")


def synthetic_data_dict(seed: int = 7) -> Dict[str, list]:
    """He-normal filters and small biases in the vgg16.npy structure."""
    rng = np.random.default_rng(seed)
    return {name: [(rng.standard_normal((3, 3, ci, co)) * np.sqrt(2.0 / (9 * ci))).astype(np.float32),
                   (rng.standard_normal(co) * 0.05).astype(np.float32)] for name, ci, co in LAYERS}


def _preprocess_launch(x):
    out = torch.empty_like(x)
    mean = (C.c_float * 4)(*VGG_MEAN, 0.0)
    runtime.call(x.device, "vstab_scale_shift", x.data_ptr(), x.numel() // 3, 3, 255.0, mean, out.data_ptr())
    return out


def _preprocess_backward(saved, dout, needs, statics):
    dout = dout.contiguous()
    dx = torch.empty_like(dout)
    runtime.call(dout.device, "vstab_axpby", dout.data_ptr(), 255.0, dout.data_ptr(), 0.0, dx.data_ptr(), dout.numel())
    return (dx,)


def preprocess(x: torch.Tensor) -> torch.Tensor:
    """NLDF.py:29: input_holder * 255. - vgg16.VGG_MEAN.  Differentiable: the gradient is 255 * dout."""
    if not x.is_cuda or x.dtype != torch.float32 or x.shape[-1] != 3:
        raise ValueError("x must be a float32 CUDA tensor [..., 3]")
    return _autograd.apply(_preprocess_launch, _preprocess_backward, (x.contiguous(),))


class _FeaturesFn(torch.autograd.Function):
    """Vgg16.features: build() forward, Vgg16._backward backward.  `handle` is the model's one-element leaf that keeps a trainable
    trunk in the graph when the input itself needs no gradient; it never receives one."""

    @staticmethod
    def forward(ctx, vgg, names, x, handle):
        vgg.build(x)
        ctx.vgg, ctx.names, ctx.last = vgg, names, vgg._last
        return tuple(getattr(vgg, n).detach() for n in names)

    @staticmethod
    @once_differentiable
    def backward(ctx, *douts):
        vgg, last = ctx.vgg, ctx.last
        if vgg._last is not last and vgg._last is not None and vgg._last["outs"] is last["outs"]:
            raise RuntimeError("Vgg16.features: backward against stale activations: with reuse_outputs=True a later build() has "
                               "overwritten the tensors this graph was recorded on")
        grads = {n: g for n, g in zip(ctx.names, douts) if g is not None}
        need_input = ctx.needs_input_grad[2]
        if not grads or not (need_input or vgg.trainable):
            return None, None, None, None
        dparams = vgg._grad_tensors(last["x"].device) if vgg.trainable else None
        dinput = vgg._backward(last, grads, need_input, dparams, accumulate=True)
        return None, None, dinput, None


class Vgg16:
    def __init__(self, vgg16_npy_path: Optional[str] = None, data_dict: Optional[dict] = None, seed: Optional[int] = None,
                 reuse_outputs: bool = False, trainable: bool = False):
        """reuse_outputs=True keeps the 18 output tensors (2.45 GB per 1080p sample) and the workspace
        between build() calls of the same shape instead of allocating them anew: the tensors a previous
        build() returned are then overwritten by the next one.
        trainable=True: a backward through features() accumulates the filter gradients into self.grads
        ({layer: (dW, db)} CUDA tensors; zero_grads() clears them, apply_grads(lr) takes an SGD step)."""
        self.reuse_outputs = reuse_outputs
        self.trainable = trainable
        self.grads: Dict[str, tuple] = {}
        self._last = None                  # what the last build() ran on: input, outputs, shape
        self._params = None                # device-resident masters of the filters, once apply_grads has stepped them
        self._handle = None
        self._cache = {}
        if data_dict is None:
            if seed is not None:
                data_dict = synthetic_data_dict(seed)
            else:
                if vgg16_npy_path is None:
                    vgg16_npy_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "vgg16.npy")
                data_dict = np.load(vgg16_npy_path, allow_pickle=True, encoding="latin1").item()
        self.data_dict = data_dict
        self._ctx = None

    def _context(self, device):
        if self._ctx is None or self._ctx.device != device:
            ctx = runtime.Context(device)
            self._load(ctx)
            self._ctx = ctx
        return self._ctx

    def _load(self, ctx):
        arr = (_lib.VstabTensor * 26)()
        keep = []
        i = 0
        for name, ci, co in LAYERS:
            if name not in self.data_dict:
                raise KeyError(f"vgg16 weights lack layer {name!r}")
            W = np.ascontiguousarray(np.asarray(self.data_dict[name][0]), dtype=np.float32)
            b = np.ascontiguousarray(np.asarray(self.data_dict[name][1]), dtype=np.float32)
            if W.shape != (3, 3, ci, co) or b.shape != (co,):
                raise ValueError(f"{name}: filter {W.shape} / biases {b.shape}, expected {(3, 3, ci, co)} / {(co,)}")
            for suffix, a in (("filter", W), ("biases", b)):
                nb = f"{name}/{suffix}".encode()
                keep.append((nb, a))
                arr[i].name = nb
                arr[i].data = a.ctypes.data_as(_lib.c_float_p)
                arr[i].ndim = a.ndim
                for d in range(a.ndim):
                    arr[i].shape[d] = a.shape[d]
                i += 1
        _lib.check(_lib.lib().vstab_vgg16_load(ctx._h, arr, 26), ctx._h)

    def build(self, input, train=False):
        """input [B,H,W,3] float32 CUDA -> sets self.conv1_1 ... self.pool5 (NHWC tensors)."""
        if not torch.is_tensor(input) or not input.is_cuda or input.dtype != torch.float32 or input.dim() != 4 \
                or input.shape[3] != 3:
            raise ValueError("input must be a float32 CUDA tensor [B,H,W,3]")
        x = input.contiguous()
        B, H, W, _ = x.shape
        ctx = self._context(x.device.index)
        L = _lib.lib()
        hwc = (C.c_int32 * 54)()
        _lib.check(L.vstab_vgg16_shapes(H, W, hwc))
        key = (B, H, W, x.device.index)
        cached = self._cache.get(key) if self.reuse_outputs else None
        if cached is None:
            outs = [torch.empty((B, hwc[3 * i], hwc[3 * i + 1], hwc[3 * i + 2]), dtype=torch.float32, device=x.device)
                    for i in range(18)]
            nws = L.vstab_vgg16_workspace_bytes(B, H, W)
            if nws == 0:
                raise ValueError(f"vgg16: unsupported problem {(B, H, W)}")
            ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
            if self.reuse_outputs:
                self._cache = {key: (outs, ws, nws)}
        else:
            outs, ws, nws = cached
        ptrs = (C.c_void_p * 18)(*[o.data_ptr() for o in outs])
        runtime.call(x.device, "vstab_vgg16_forward", ctx._h, x.data_ptr(), B, H, W, ptrs, ws.data_ptr(), nws, ctx=ctx._h)
        for name, t in zip(OUTPUTS, outs):
            setattr(self, name, t)
        self._last = {"x": x, "outs": outs, "shape": (B, H, W)}
        return self

    # ---- backward
    def _backward(self, last, grads, need_input, dparams, accumulate):
        """The C walk on the activations `last` recorded.  dparams: 26 tensors in LAYERS order (filter, biases) or None."""
        x, outs = last["x"], last["outs"]
        B, H, W = last["shape"]
        if not grads:
            raise ValueError("grads is empty: no output carries a gradient")
        held = []
        dptr = (C.c_void_p * 18)()
        for name, g in grads.items():
            if name not in OUTPUTS:
                raise ValueError(f"{name!r} is not one of vgg16.OUTPUTS")
            o = outs[OUTPUTS.index(name)]
            if not torch.is_tensor(g) or g.dtype != torch.float32 or g.device != o.device or g.shape != o.shape:
                raise ValueError(f"grads[{name!r}] must be a float32 tensor of shape {tuple(o.shape)} on {o.device}")
            g = g.contiguous()
            held.append(g)
            dptr[OUTPUTS.index(name)] = g.data_ptr()
        if not need_input and dparams is None:
            raise ValueError("neither the input gradient nor the filter gradients are asked for")
        ctx = self._context(x.device.index)
        dinput = torch.empty_like(x) if need_input else None
        optr = (C.c_void_p * 18)(*[o.data_ptr() for o in outs])
        pptr = (C.c_void_p * 26)(*[p.data_ptr() for p in dparams]) if dparams is not None else None
        with torch.cuda.device(x.device):
            ws = runtime.workspace(x.device, "vstab_vgg16_backward_workspace_bytes", B, H, W, 1 if dparams is not None else 0,
                                   refused=f"vgg16 backward: unsupported problem {(B, H, W)}")
        runtime.call(x.device, "vstab_vgg16_backward", ctx._h, x.data_ptr(), B, H, W, optr, dptr, runtime.ptr(dinput), pptr,
                     1 if accumulate else 0, ws.data_ptr(), ws.numel(), ctx=ctx._h)
        return dinput

    def backward(self, grads: Dict[str, torch.Tensor], need_input: bool = True, need_weights: bool = False):
        """Pulls `grads` ({name in OUTPUTS: gradient of that output}) back through the activations of the last build():
        (dinput [B,H,W,3] or None, {layer: (dW [3,3,Cin,Cout], db [Cout])} or None).  Layers above the deepest output named
        are not touched; their filter gradients are zero."""
        if self._last is None:
            raise RuntimeError("Vgg16.backward: build() has not been called")
        dev = self._last["x"].device
        dparams = None
        if need_weights:
            dparams = [t for _, ci, co in LAYERS for t in (torch.zeros((3, 3, ci, co), dtype=torch.float32, device=dev),
                                                           torch.zeros(co, dtype=torch.float32, device=dev))]
        dinput = self._backward(self._last, grads, need_input, dparams, accumulate=False)
        if dparams is None:
            return dinput, None
        return dinput, {name: (dparams[2 * i], dparams[2 * i + 1]) for i, (name, _, _) in enumerate(LAYERS)}

    def features(self, input, names: Sequence[str]):
        """build(input) under torch.autograd: the outputs `names` (of OUTPUTS) as a tuple attached to the graph.  Their backward
        gives d/d input when input.requires_grad and, for a trainable model, accumulates the filter gradients into self.grads."""
        names = tuple(names)
        if not names or len(set(names)) != len(names) or any(n not in OUTPUTS for n in names):
            raise ValueError(f"names must be distinct members of vgg16.OUTPUTS, got {names!r}")
        x = runtime.f32_cuda(input, "input", rank=4, last=3, layout="[B,H,W,3]")
        if not torch.is_grad_enabled() or not (x.requires_grad or self.trainable):
            self.build(x)
            return tuple(getattr(self, n) for n in names)
        if self._handle is None or self._handle.device != x.device:
            self._handle = torch.zeros(1, dtype=torch.float32, device=x.device, requires_grad=True)
        return _FeaturesFn.apply(self, names, x, self._handle)

    def _grad_tensors(self, device):
        if not self.grads or next(iter(self.grads.values()))[0].device != device:
            self.grads = {name: (torch.zeros((3, 3, ci, co), dtype=torch.float32, device=device),
                                 torch.zeros(co, dtype=torch.float32, device=device)) for name, ci, co in LAYERS}
        return [t for name, _, _ in LAYERS for t in self.grads[name]]

    def zero_grads(self):
        for dW, db in self.grads.values():
            dW.zero_()
            db.zero_()

    def export(self) -> Dict[str, list]:
        """The filters in the vgg16.npy structure ({layer: [W, b]} numpy): the stepped ones once apply_grads has run."""
        if self._params is None:
            return {name: [np.asarray(self.data_dict[name][0], dtype=np.float32), np.asarray(self.data_dict[name][1], dtype=np.float32)]
                    for name, _, _ in LAYERS}
        return {name: [W.cpu().numpy(), b.cpu().numpy()] for name, (W, b) in self._params.items()}

    def load(self, data_dict: dict):
        """Replaces the filters (vgg16.npy structure) and re-packs them on the device of the current context."""
        self.data_dict = data_dict
        self._params = None
        if self._ctx is not None:
            self._load(self._ctx)

    def apply_grads(self, lr: float):
        """One plain SGD step p -= lr * grad on device-resident masters of the filters (vstab_axpby).  The packed and Winograd
        forms the forward reads are built by the host packers of vstab_vgg16_load, so the stepped filters then go through
        export() and load()."""
        if not self.grads:
            raise RuntimeError("Vgg16.apply_grads: no gradients (trainable=True and a backward through features() fill them)")
        dev = next(iter(self.grads.values()))[0].device
        if self._params is None or next(iter(self._params.values()))[0].device != dev:
            host = self.export() if self._params is not None else None
            self._params = {name: tuple(torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev)
                                        for a in (host or self.data_dict)[name][:2]) for name, _, _ in LAYERS}
        for name, _, _ in LAYERS:
            for p, g in zip(self._params[name], self.grads[name]):
                runtime.call(dev, "vstab_axpby", p.data_ptr(), 1.0, g.data_ptr(), -float(lr), p.data_ptr(), p.numel())
        params = self._params
        self.load(self.export())
        self._params = params

    def L2(self, tensor, wd=0.001):
        """vgg16.py:99-100: wd * sum(tensor^2) / 2 of a float32 CUDA tensor (the product the reference's `tf.mul`, gone from TF 1.x,
        names), a 0-dim tensor.  Differentiable; summed in a fixed order (nldf_loss.py)."""
        return nldf_loss.l2(tensor, wd)
