"""Inference forward of the theta regressors (theta_nets.py) over the C ABI: vstab_pad_symmetric -> vstab_conv_forward (pad 0, no
activation) -> vstab_bn_lrelu_slope_inference / ..._pool_inference per convolution, then vstab_dense_forward per dense layer.

One `ThetaNet` per (builder, scope, device) keeps the variables on the device, uploaded once, in the layouts the kernels read: the
filters with their input channels zero-padded to a multiple of 4 (the staged input's channel stride), the dense matrices as the
reference stores them.  Activation buffers and workspaces are cached per input shape; a forward enqueues launches on the current
stream and never synchronises."""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from . import _lib, runtime, theta_nets
from .runtime import _up4

DENSE_ACT = {"identity": 0, "lrelu": 1, "tanh": 2, "tanh_affine": 3}          # VSTAB_DENSE_*



# ---- one wrapper per entry point (tests and benchmarks; ThetaNet.forward issues the same calls on its cached buffers)
def pad_symmetric(x: torch.Tensor, p: int, cs: Optional[int] = None) -> torch.Tensor:
    """tf.pad(x, SYMMETRIC) of x [B,H,W,C] by p rows and columns into a channel stride `cs` (default: C rounded up to 4)"""
    x = runtime.f32_cuda(x, "x", 4, layout="[B,H,W,C]")
    B, H, W, C = x.shape
    cs = _up4(C) if cs is None else int(cs)
    y = torch.empty((B, H + 2 * p, W + 2 * p, cs), dtype=torch.float32, device=x.device)
    runtime.call(x.device, "vstab_pad_symmetric", x.data_ptr(), B, H, W, C, int(p), y.data_ptr(), cs)
    return y


def bn_lrelu_slope_inference(z: torch.Tensor, beta, moving_mean, moving_var, slope: float = theta_nets.LRELU_SLOPE, twice: bool = False,
                             eps: float = theta_nets.BN_EPS, c_off: int = 0, C: Optional[int] = None) -> torch.Tensor:
    """In place on channels c_off..c_off+C of z [..., cs]; returns z."""
    z = runtime.f32_cuda(z, "z", layout="[..., cs]")
    cs = z.shape[-1]
    C = cs - c_off if C is None else C
    runtime.call(z.device, "vstab_bn_lrelu_slope_inference", z.data_ptr(), z.numel() // cs, cs, c_off, C, beta.data_ptr(), moving_mean.data_ptr(),
                 moving_var.data_ptr(), eps, slope, int(bool(twice)))
    return z


def bn_lrelu_slope_pool_inference(z: torch.Tensor, beta, moving_mean, moving_var, slope: float = theta_nets.LRELU_SLOPE, twice: bool = False,
                                  eps: float = theta_nets.BN_EPS) -> torch.Tensor:
    """z [B,H,W,C] -> the layer's output after MaxPool2d(2, 2, SAME), [B,ceil(H/2),ceil(W/2),C]; z is not written."""
    z = runtime.f32_cuda(z, "z", 4, layout="[B,H,W,C]")
    B, H, W, C = z.shape
    out = torch.empty((B, (H + 1) // 2, (W + 1) // 2, C), dtype=torch.float32, device=z.device)
    runtime.call(z.device, "vstab_bn_lrelu_slope_pool_inference", z.data_ptr(), B, H, W, C, beta.data_ptr(), moving_mean.data_ptr(),
                 moving_var.data_ptr(), eps, slope, int(bool(twice)), out.data_ptr())
    return out


def dense_forward(x: torch.Tensor, W: torch.Tensor, b: torch.Tensor, act: str = "identity", slope: float = theta_nets.LRELU_SLOPE,
                  scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(x [B,K] . W [K,N] + b); `scale`, `shift` [N] with act='tanh_affine'"""
    x = runtime.f32_cuda(x, "x", 2, layout="[B,K]")
    W = runtime.f32_cuda(W, "W", 2, layout="[K,N]")
    (B, K), N = x.shape, W.shape[1]
    if W.shape[0] != K or tuple(b.shape) != (N,):
        raise ValueError(f"dense_forward: x {tuple(x.shape)}, W {tuple(W.shape)}, b {tuple(b.shape)}")
    ws = runtime.workspace(x.device, "vstab_dense_forward_workspace_bytes", B, K, N,
                           refused=f"dense_forward takes no B={B}, K={K}, N={N} (1 <= B <= 32, K a multiple of 4)")
    y = torch.empty((B, N), dtype=torch.float32, device=x.device)
    runtime.call(x.device, "vstab_dense_forward", x.data_ptr(), B, K, N, W.data_ptr(), b.data_ptr(), DENSE_ACT[act], slope, runtime.ptr(scale),
                 runtime.ptr(shift), y.data_ptr(), ws.data_ptr(), ws.numel())
    return y


class ThetaNet:
    def __init__(self, net: str, device: int, weights: Dict[str, np.ndarray]):
        runtime._require_gpu()
        self.graph = theta_nets.graph(net)
        self.device = torch.device("cuda", device)
        self._bufs: Dict[tuple, dict] = {}
        self.load_weights(weights)

    def load_weights(self, w: Dict[str, np.ndarray]):
        """`w`: theta_nets.validate's output.  The dead layers' variables are not uploaded."""
        g = self.graph
        self.cin = int(w[f"{g.convs[0].name}/W_conv2d"].shape[2])
        self.flat = int(w[f"{g.dense[0].name}/W"].shape[0])
        self.units = tuple(int(w[f"{d.name}/W"].shape[1]) for d in g.dense)
        dev = {}
        for name in g.live_names(w):
            a = w[name]
            if name.endswith("/W_conv2d") and a.shape[2] % 4:
                padded = np.zeros((3, 3, _up4(a.shape[2]), a.shape[3]), np.float32)
                padded[:, :, :a.shape[2]] = a
                a = padded
            dev[name] = torch.from_numpy(a).to(self.device)
        dev["homo_scale"] = torch.tensor(theta_nets.HOMO_SCALE, dtype=torch.float32, device=self.device)
        dev["homo_shift"] = torch.tensor(theta_nets.HOMO_SHIFT, dtype=torch.float32, device=self.device)
        self._dev = dev
        self._bufs.clear()

    def _buffers(self, B: int, H: int, W: int) -> dict:
        key = (B, H, W)
        b = self._bufs.get(key)
        if b is not None:
            return b
        g, L = self.graph, _lib.lib()
        sz = g.sizes_for(H, W)
        if sz.flat != self.flat:
            raise ValueError(f"{g.name}: a {H}x{W} input flattens to {sz.flat} features, but the assigned {g.dense[0].name}/W has "
                             f"{self.flat} rows")
        if not 1 <= B <= 32:
            raise ValueError(f"{g.name}: batch {B} outside 1..32")

        def f32(*shape):
            return torch.empty(shape, dtype=torch.float32, device=self.device)

        stages, conv_ws, h, w, c = [], 0, H, W, self.cin
        for i, st in enumerate(g.convs):
            cs = _up4(c)
            staged = st.sym_pad > 0 or c != cs          # Localizer's later layers read the previous activation where it lies
            hi, wi = h + 2 * st.sym_pad, w + 2 * st.sym_pad
            ho, wo = sz.conv[i]
            n = int(L.vstab_conv_forward_workspace_bytes(B, hi, wi, cs, cs, 3, st.stride, 0, st.cout, st.cout, 0, 0, ho, wo))
            if n == 0:
                raise _lib.VstabError(f"{g.name}: vstab_conv_forward takes no B={B} {hi}x{wi} {cs}->{st.cout} stride-{st.stride} convolution")
            conv_ws = max(conv_ws, n)
            stages.append(dict(st=st, h=h, w=w, c=c, cs=cs, hi=hi, wi=wi, ho=ho, wo=wo, xp=f32(B, hi, wi, cs) if staged else None,
                               z=f32(B, ho, wo, st.cout), pooled=f32(B, *sz.out[i], st.cout) if st.pool else None))
            (h, w), c = sz.out[i], st.cout
        dense_ws, k = 0, sz.flat
        for n in self.units:
            dense_ws = max(dense_ws, int(L.vstab_dense_forward_workspace_bytes(B, k, n)))
            k = n
        b = dict(stages=stages, conv_ws=torch.empty(max(conv_ws, 256), dtype=torch.uint8, device=self.device),
                 dense_ws=torch.empty(max(dense_ws, 256), dtype=torch.uint8, device=self.device),
                 hidden=[f32(B, n) for n in self.units[:-1]])
        self._bufs[key] = b
        return b

    def forward(self, feats: torch.Tensor, last_act: Optional[str] = None) -> torch.Tensor:
        """feats [B,H,W,cin] -> [B, units of the last dense layer]; `last_act` replaces the last dense layer's activation (Localizer's
        is_tanh).  feats is read only."""
        g, p, dev = self.graph, self._dev, self.device
        feats = runtime.f32_cuda(feats, "feats", 4, layout="[B,H,W,C]")
        if feats.device != dev:
            raise ValueError(f"feats is on {feats.device}, the weights on {dev}")
        B, H, W, C = feats.shape
        if C != self.cin:
            raise ValueError(f"{g.name}: feats has {C} channels, the assigned {g.convs[0].name}/W_conv2d takes {self.cin}")
        b = self._buffers(B, H, W)
        eps, slope = theta_nets.BN_EPS, theta_nets.LRELU_SLOPE
        x, ws = feats, b["conv_ws"]
        for s in b["stages"]:
            st = s["st"]
            if s["xp"] is not None:
                runtime.call(dev, "vstab_pad_symmetric", x.data_ptr(), B, s["h"], s["w"], s["c"], st.sym_pad, s["xp"].data_ptr(), s["cs"])
                x = s["xp"]
            runtime.call(dev, "vstab_conv_forward", x.data_ptr(), B, s["hi"], s["wi"], s["cs"], 0, s["cs"], p[f"{st.name}/W_conv2d"].data_ptr(),
                         p[f"{st.name}/b_conv2d"].data_ptr(), 3, st.stride, 0, s["z"].data_ptr(), s["ho"], s["wo"], st.cout, 0, st.cout, 0,
                         ws.data_ptr(), ws.numel())
            bn = [p[f"{st.bn}/{v}"].data_ptr() for v in ("beta", "moving_mean", "moving_variance")]
            if st.pool:
                runtime.call(dev, "vstab_bn_lrelu_slope_pool_inference", s["z"].data_ptr(), B, s["ho"], s["wo"], st.cout, *bn, eps, slope, 0,
                             s["pooled"].data_ptr())
                x = s["pooled"]
            else:
                runtime.call(dev, "vstab_bn_lrelu_slope_inference", s["z"].data_ptr(), B * s["ho"] * s["wo"], st.cout, 0, st.cout, *bn, eps,
                             slope, 0)
                x = s["z"]
        out = torch.empty((B, self.units[-1]), dtype=torch.float32, device=dev)
        k, ws = self.flat, b["dense_ws"]
        for i, (d, n) in enumerate(zip(g.dense, self.units)):
            last = i == len(g.dense) - 1
            y = out if last else b["hidden"][i]
            act = last_act if last and last_act is not None else d.act
            # DenseLayer(lrelu) -> BatchNormLayer(lrelu): the dense launch adds the bias, the epilogue applies the activation on both sides
            fused = d.bn is not None and act == "lrelu"
            runtime.call(dev, "vstab_dense_forward", x.data_ptr(), B, k, n, p[f"{d.name}/W"].data_ptr(), p[f"{d.name}/b"].data_ptr(),
                         DENSE_ACT["identity" if fused else act], slope, p["homo_scale"].data_ptr(), p["homo_shift"].data_ptr(), y.data_ptr(),
                         ws.data_ptr(), ws.numel())
            if d.bn is not None:
                bn = [p[f"{d.bn}/{v}"].data_ptr() for v in ("beta", "moving_mean", "moving_variance")]
                runtime.call(dev, "vstab_bn_lrelu_slope_inference", y.data_ptr(), B, n, 0, n, *bn, eps, slope, 1 if fused else 0)
            x, k = y, n
        return out


# ---- registry: host variables per (graph, scope), device nets per (graph, scope, device)
_pending: Dict[Tuple[str, str], Dict[str, np.ndarray]] = {}
_nets: Dict[Tuple[str, str, int], ThetaNet] = {}


def assign_weights(net: str, weights: Dict[str, np.ndarray], scope: Optional[str] = None) -> Dict[str, np.ndarray]:
    """Register the variables of builder `net` under `scope` (its default scope when None); short names or checkpoint keys."""
    g = theta_nets.graph(net)
    scope = scope or g.scope
    w = theta_nets.validate(net, weights, scope)
    _pending[(g.name, scope)] = w
    for (name, sc, _dev), tn in _nets.items():
        if (name, sc) == (g.name, scope):
            tn.load_weights(w)
    return w


def get_net(net: str, scope: str, device: Optional[int] = None) -> ThetaNet:
    runtime._require_gpu()
    g = theta_nets.graph(net)
    if device is None:
        device = torch.cuda.current_device()
    key = (g.name, scope, device)
    tn = _nets.get(key)
    if tn is None:
        if (g.name, scope) not in _pending:
            raise RuntimeError(f"vstab: no weights assigned for {g.name} under scope {scope!r} (initialize_global_variables / "
                               f"load_and_assign_npz_dict / assign_weights with net={g.name!r})")
        tn = _nets[key] = ThetaNet(net, device, _pending[(g.name, scope)])
    return tn


def reset():
    _pending.clear()
    _nets.clear()
