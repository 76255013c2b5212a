"""Drop-in for the reference's cell.py: ConvLSTMCell (cell.py:5-76) and ConvGRUCell (cell.py:78-136) on float32 CUDA tensors in NHWC.

By default forward only: results carry no `grad_fn`, whatever the inputs require (as the bicubic sampler's).  Built with
`differentiable=True` a cell trains (last paragraph).  A step is the SAME convolution over
concat([x, h]) on the MFMA implicit-GEMM kernel (`vstab_conv_forward`) followed by the fused gate launches of csrc/cell_ops.hip
(`vstab_convlstm_gates`, `vstab_convgru_gates`, `vstab_convgru_update`).  x and h live side by side in one persistent NHWC buffer per
cell and batch size whose channel stride and h offset are rounded up to multiples of 4 (pad channels zero, the kernel tensor padded
to match once, in `assign_weights`); the gate kernel writes the new h straight into that buffer's slice (the GRU: r*h into the slice
of a second buffer), so no concat is ever copied.

Arithmetic (tests/cell_ref.py restates it index by index):
  LSTM  y = conv(concat(x, h), kernel) [+ bias unless normalize];  j, i, f, o = the four F-channel blocks of y;
        peephole: i += W_ci c, f += W_cf c;  normalize: j, i, f = LN;  f = sigmoid(f + forget_bias), i = sigmoid(i);
        c' = c f + i act(j);  peephole: o += W_co c';  normalize: o = LN(o), c' = LN(c');  h' = sigmoid(o) act(c');  returns (h', (c', h')).
  GRU   y = conv(concat(x, h), gates/kernel);  normalize: r, u = LN of the two blocks, else y += gates/bias;  r, u = sigmoid;
        y2 = conv(concat(x, r h), candidate/kernel);  normalize: LN(y2), else + candidate/bias;  h' = u h + (1 - u) act(y2).
  LN    tf.contrib.layers.layer_norm's defaults: per sample over all of H, W and the gate's F channels, biased variance,
        (v - mean) rsqrt(var + 1e-12) gamma[ch] + beta[ch].
        (warning: recalled from TensorFlow 1.10's source, as is the order of the LSTM's LayerNorm variables below -- SURVEY.md Appendix A.)

Weights are given, not created: `assign_weights(dict)` with the names TensorFlow gives the variables inside the cell's scope.
  LSTM  kernel [k,k,Cx+F,4F];  bias [4F] (normalize=False);  W_ci, W_cf, W_co [H,W,F] (peephole);
        LayerNorm/{gamma,beta}, LayerNorm_1/.. LayerNorm_4/.. [F] in call order j, i, f, o, c (normalize).
  GRU   gates/kernel [k,k,Cx+F,2F];  candidate/kernel [k,k,Cx+F,F];  normalize: gates/LayerNorm{,_1}/{gamma,beta} (r, u),
        candidate/LayerNorm/{gamma,beta};  else gates/bias [2F], candidate/bias [F].
`filters == 1` is the same formulas (the reference's m = 4 and m = 2).

Differentiable mode (constructor keyword `differentiable=True`; the default path is untouched): `assign_weights` (re)creates
`parameters()`, a dict name -> float32 CUDA leaf with requires_grad in the reference's shapes; every `call` / `run_sequence` reads their
current values (the padded device copies are rebuilt once per call, not per step), so an optimiser's in-place step takes effect.  When
grad mode is on and x, the state or a parameter requires grad, the results hang on one torch.autograd.Function per `call` /
`run_sequence` (the whole sequence: back-propagation through time inside it); gradients flow to the inputs, the initial state and every
parameter, `needs_input_grad` decides what is computed, forward values are bit-equal to the default path's.  Backward of a step: the
gate-stage backward kernels of csrc/cell_ops.hip (`cell_grad.convlstm_gates_backward`, `convgru_update_backward`,
`convgru_gates_backward`), then `training.conv_wgrad` and `training.conv_dgrad` on the concat buffer.  First derivatives only.

Not built: data_format='channels_first' (the reference passes 'NC' with feature axis 0 for it, which is wrong for a
batched tensor: NotImplementedError here), even or rectangular kernels, kernels wider than 7, and the commented-out
spatial-transformer GRU of cell.py:138-208.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _lib, runtime, training
from .runtime import _up4

LSTMStateTuple = collections.namedtuple("LSTMStateTuple", ("c", "h"))

_ACT_CODES = {"tanh": 0, "relu": 1, "identity": 2}
_LSTM_LN = ("LayerNorm", "LayerNorm_1", "LayerNorm_2", "LayerNorm_3", "LayerNorm_4")        # j, i, f, o, c


def _act_code(activation) -> int:
    if activation is None:
        return 2
    if isinstance(activation, str) and activation in _ACT_CODES:
        return _ACT_CODES[activation]
    if activation is torch.tanh:
        return 0
    if activation is torch.relu:
        return 1
    raise NotImplementedError(f"activation {activation!r}: 'tanh', 'relu' or 'identity' (torch.tanh, torch.relu, None)")


def _as_f32(value, name, shape):
    a = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(a.shape)}, expected {tuple(shape)}")
    return np.ascontiguousarray(a, dtype=np.float32)


class _Buffers:
    """What a cell keeps on the device for one batch size."""


class _ConvCell:
    def __init__(self, shape, filters, kernel, activation, normalize, data_format, differentiable=False):
        if data_format == "channels_first":
            raise NotImplementedError("data_format='channels_first' is not built (the reference's own form of it is wrong for a batch)")
        if data_format != "channels_last":
            raise ValueError("Unknown data_format")
        shape, kernel = list(shape), list(kernel)
        if len(shape) != 2 or min(shape) < 1:
            raise ValueError("shape must be [H, W]")
        if len(kernel) != 2 or kernel[0] != kernel[1] or kernel[0] % 2 != 1 or not 1 <= kernel[0] <= 7:
            raise NotImplementedError(f"kernel {kernel}: square, odd, at most 7")
        if int(filters) < 1:
            raise ValueError("filters must be >= 1")
        self._H, self._W = int(shape[0]), int(shape[1])
        self._filters = int(filters)
        self._k = int(kernel[0])
        self._act = _act_code(activation)
        self._normalize = bool(normalize)
        self._size = torch.Size([self._H, self._W, self._filters])
        self._cx = None                       # input channels: known once the weights are
        self._dev = {}                        # device tensors of the weights
        self._bufs = {}
        self._differentiable = bool(differentiable)
        self._params = None                   # differentiable: name -> float32 CUDA leaf, the reference's shapes

    @property
    def output_size(self):
        return self._size

    def __call__(self, x, state):
        return self.call(x, state)

    # ---- weights
    def _take(self, weights, name, shape):
        if name not in weights:
            raise ValueError(f"missing weight {name!r}")
        return _as_f32(weights[name], name, shape)

    def _kernel_in_channels(self, weights, name, m):
        if name not in weights:
            raise ValueError(f"missing weight {name!r}")
        s = tuple(weights[name].shape)
        F, k = self._filters, self._k
        if len(s) != 4 or s[0] != k or s[1] != k or s[3] != m or s[2] <= F:
            raise ValueError(f"{name}: shape {s}, expected [{k},{k},Cx+{F},{m}]")
        return s[2] - F

    def _padded_kernel(self, w, cx):
        """[k,k,Cx+F,m] -> [k,k,cs,m] with the x rows at 0 and the h rows at the padded offset, zeros between"""
        k, F = self._k, self._filters
        hoff = _up4(cx)
        out = np.zeros((k, k, hoff + _up4(F), w.shape[3]), np.float32)
        out[:, :, :cx] = w[:, :, :cx]
        out[:, :, hoff:hoff + F] = w[:, :, cx:]
        return out

    def _set_weights(self, cx, host):
        runtime._require_gpu()
        self._cx, self._hoff, self._cs = cx, _up4(cx), _up4(cx) + _up4(self._filters)
        self._dev = {n: torch.from_numpy(a).cuda() for n, a in host.items()}
        self._bufs = {}

    def _ptr(self, name):
        t = self._dev.get(name)
        return t.data_ptr() if t is not None else None

    # ---- differentiable mode
    def parameters(self):
        """name -> tensor with the names and shapes of `weight_shapes()`: float32 CUDA leaves with requires_grad, (re)created by
        `assign_weights`.  Every `call` / `run_sequence` reads their current values."""
        if not self._differentiable:
            raise ValueError("parameters(): construct the cell with differentiable=True")
        if self._params is None:
            raise ValueError("assign_weights() first")
        return dict(self._params)

    def _set_parameters(self, cx, host):
        runtime._require_gpu()
        self._cx, self._hoff, self._cs = cx, _up4(cx), _up4(cx) + _up4(self._filters)
        self._params = {n: torch.from_numpy(a).cuda().requires_grad_() for n, a in host.items()}
        self._bufs = {}
        self._refresh()

    def _padded_kernel_dev(self, w):
        """`_padded_kernel` on the device, twice: ([k,k,cs,m] for the forward, the same with the output channels zero-padded to a
        multiple of 4 for `vstab_conv_dgrad`)"""
        k, F, cx, m = self._k, self._filters, self._cx, w.shape[3]
        out = torch.zeros((k, k, self._cs, _up4(m)), dtype=torch.float32, device=w.device)
        out[:, :, :cx, :m] = w[:, :, :cx]
        out[:, :, self._hoff:self._hoff + F, :m] = w[:, :, cx:]
        return (out if m % 4 == 0 else out[..., :m].contiguous()), out

    def _refresh(self):
        """the device copies the kernels read, from the parameters' current values: once per call / run_sequence"""
        with torch.no_grad():
            self._dev = self._dev_from({n: t.detach() for n, t in self._params.items()})

    def _wants_graph(self, *tensors):
        return torch.is_grad_enabled() and any(t.requires_grad for t in tensors + tuple(self._params.values()))

    def _kernel_grad(self, dW):
        """[k,k,cs,m] in the concat layout -> the reference's [k,k,Cx+F,m]"""
        return torch.cat([dW[:, :, :self._cx], dW[:, :, self._hoff:self._hoff + self._filters]], dim=2)

    def _stats(self, ws, offset, Q, B):
        return ws[offset:offset + B * Q * 8].clone()

    # ---- checks
    def _check_tensor(self, t, name, channels):
        if not torch.is_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
            raise ValueError(f"{name} must be a float32 CUDA tensor")
        if t.dim() != 4 or tuple(t.shape[1:]) != (self._H, self._W, channels):
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected [B,{self._H},{self._W},{channels}]")

    def _check_call(self, x, states):
        if self._cx is None:
            raise ValueError("assign_weights() first")
        self._check_tensor(x, "x", self._cx)
        for name, s in states:
            self._check_tensor(s, name, self._filters)
            if s.shape[0] != x.shape[0] or s.device != x.device:
                raise ValueError(f"{name}: batch / device differ from x's")
        if x.device != next(iter(self._dev.values())).device:
            raise ValueError("x is not on the device of the weights")

    # ---- convolution over a concat buffer
    def _conv_ws_bytes(self, B, m):
        n = int(_lib.lib().vstab_conv_forward_workspace_bytes(B, self._H, self._W, self._cs, self._cs, self._k, 1, (self._k - 1) // 2, m, _up4(m),
                                                              0, 0, self._H, self._W))
        if n == 0:
            raise _lib.VstabError(f"vstab_conv_forward takes no B={B} {self._H}x{self._W} {self._cs}->{m} k={self._k} convolution")
        return n

    def _conv(self, cat, w, bias, y, m, ws):
        B = cat.shape[0]
        _lib.check(_lib.lib().vstab_conv_forward(cat.data_ptr(), B, self._H, self._W, self._cs, 0, self._cs, w.data_ptr(),
                                                 bias.data_ptr() if bias is not None else None, self._k, 1, (self._k - 1) // 2, y.data_ptr(),
                                                 self._H, self._W, _up4(m), 0, m, 0, ws.data_ptr(), ws.numel(), runtime.stream_ptr()))

    def _new_cat(self, B, device):
        return torch.zeros((B, self._H, self._W, self._cs), dtype=torch.float32, device=device)

    def _h_slice_ptr(self, cat):
        return cat.data_ptr() + 4 * self._hoff

    def _new_state(self, B, device):
        return torch.empty((B, self._H, self._W, self._filters), dtype=torch.float32, device=device)

    def buffers(self, B, device):
        """The persistent device buffers for batch size B (made on first use): concat buffer(s) `cat`, convolution output(s) `y`,
        workspaces `conv_ws`, `gate_ws`."""
        key = (int(B), torch.device(device))
        if key not in self._bufs:
            with torch.cuda.device(device):
                self._bufs[key] = self._make_buffers(int(B), torch.device(device))
        return self._bufs[key]


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


class ConvLSTMCell(_ConvCell):
    """The reference's ConvLSTMCell (cell.py:5-76); module docstring.  `call(x, (c, h))` returns `(h', LSTMStateTuple(c', h'))` as new
    tensors without `grad_fn`."""

    def __init__(self, shape, filters, kernel, forget_bias=1.0, activation="tanh", normalize=True, peephole=True, data_format="channels_last",
                 reuse=None, differentiable=False):
        super().__init__(shape, filters, kernel, activation, normalize, data_format, differentiable)
        self._forget_bias = float(forget_bias)
        self._peephole = bool(peephole)

    @property
    def state_size(self):
        return LSTMStateTuple(self._size, self._size)

    def weight_shapes(self, in_channels):
        F, k, H, W = self._filters, self._k, self._H, self._W
        s = {"kernel": (k, k, in_channels + F, 4 * F)}
        if not self._normalize:
            s["bias"] = (4 * F,)
        if self._peephole:
            s.update({n: (H, W, F) for n in ("W_ci", "W_cf", "W_co")})
        if self._normalize:
            for ln in _LSTM_LN:
                s[ln + "/gamma"] = s[ln + "/beta"] = (F,)
        return s

    def assign_weights(self, weights):
        cx = self._kernel_in_channels(weights, "kernel", 4 * self._filters)
        host = {n: self._take(weights, n, s) for n, s in self.weight_shapes(cx).items()}
        if self._differentiable:
            return self._set_parameters(cx, host)
        dev = {"kernel": self._padded_kernel(host["kernel"], cx)}
        for n in ("bias", "W_ci", "W_cf", "W_co"):
            if n in host:
                dev[n] = host[n]
        if self._normalize:
            dev["gamma"] = np.stack([host[ln + "/gamma"] for ln in _LSTM_LN])
            dev["beta"] = np.stack([host[ln + "/beta"] for ln in _LSTM_LN])
        self._set_weights(cx, dev)

    def _dev_from(self, p):
        dev = {n: p[n].contiguous() for n in ("bias", "W_ci", "W_cf", "W_co") if n in p}
        dev["kernel"], dev["kernel4"] = self._padded_kernel_dev(p["kernel"])
        if self._normalize:
            dev["gamma"] = torch.stack([p[ln + "/gamma"] for ln in _LSTM_LN])
            dev["beta"] = torch.stack([p[ln + "/beta"] for ln in _LSTM_LN])
        return dev

    def synthetic_weights(self, seed, in_channels, random_ln=False):
        """Weights for tests and the benchmark as a dict of numpy arrays: the kernel scaled so that pre-activations of U(-1,1) inputs are
        O(1), peepholes U(-0.5,0.5), the reference's initialisers where it states them (bias zeros; gamma ones and beta zeros unless
        random_ln)."""
        return _synthetic(self.weight_shapes(in_channels), seed, random_ln, {})

    def _make_buffers(self, B, device):
        F, m = self._filters, 4 * self._filters
        L = _lib.lib()
        b = _Buffers()
        b.cat = self._new_cat(B, device)
        b.y = torch.empty((B, self._H, self._W, _up4(m)), dtype=torch.float32, device=device)
        b.conv_ws = _ws(self._conv_ws_bytes(B, m), device)
        b.gate_ws = _ws(L.vstab_convlstm_gates_workspace_bytes(B, self._H, self._W, F, int(self._normalize)), device)
        return b

    def _step(self, b, c, c_out, h_out):
        """one step on loaded buffers: b.cat holds x and h; c [B,H,W,F] -> c_out (may be c), h_out and the h slice of b.cat"""
        self._conv(b.cat, self._dev["kernel"], self._dev.get("bias"), b.y, 4 * self._filters, b.conv_ws)
        self._gates(b, c, c_out, h_out)

    def _gates(self, b, c, c_out, h_out):
        _lib.check(_lib.lib().vstab_convlstm_gates(
            b.y.data_ptr(), b.y.shape[3], c.data_ptr(), self._ptr("W_ci"), self._ptr("W_cf"), self._ptr("W_co"), self._ptr("gamma"),
            self._ptr("beta"), c.shape[0], self._H, self._W, self._filters, self._forget_bias, self._act, int(self._normalize),
            int(self._peephole), c_out.data_ptr(), h_out.data_ptr(), self._h_slice_ptr(b.cat), self._cs, b.gate_ws.data_ptr(), b.gate_ws.numel(),
            runtime.stream_ptr()))

    def call(self, x, state):
        try:
            c, h = state
        except (TypeError, ValueError):
            raise ValueError("state must be a (c, h) pair") from None
        self._check_call(x, (("c", c), ("h", h)))
        if self._differentiable:
            self._refresh()
            if self._wants_graph(x, c, h):
                with torch.cuda.device(x.device):
                    outs, c_new = _LstmSequence.apply(self, x.unsqueeze(0), c, h, *self._params.values())
                h_new = outs[0]
                return h_new, LSTMStateTuple(c_new, h_new)
        with torch.no_grad(), torch.cuda.device(x.device):
            b = self.buffers(x.shape[0], x.device)
            b.cat[..., :self._cx].copy_(x)
            b.cat[..., self._hoff:self._hoff + self._filters].copy_(h)
            c_new, h_new = self._new_state(x.shape[0], x.device), self._new_state(x.shape[0], x.device)
            self._step(b, c.detach().contiguous(), c_new, h_new)
        return h_new, LSTMStateTuple(c_new, h_new)

    def _sequence(self, inputs, state):
        T, B = inputs.shape[0], inputs.shape[1]
        b = self.buffers(B, inputs.device)
        outputs = torch.empty((T, B) + tuple(self._size), dtype=torch.float32, device=inputs.device)
        hs = b.cat[..., self._hoff:self._hoff + self._filters]
        if state is None:
            c = torch.zeros_like(outputs[0])
            hs.zero_()
        else:
            c = state[0].detach().clone()
            hs.copy_(state[1])
        for t in range(T):
            b.cat[..., :self._cx].copy_(inputs[t])
            self._step(b, c, c, outputs[t])
        return outputs, LSTMStateTuple(c, outputs[T - 1].clone())

    def _sequence_graph(self, inputs, state):
        if state is None:
            c0 = h0 = torch.zeros((inputs.shape[1],) + tuple(self._size), dtype=torch.float32, device=inputs.device)
        else:
            c0, h0 = state
        outputs, c = _LstmSequence.apply(self, inputs, c0, h0, *self._params.values())
        return outputs, LSTMStateTuple(c, outputs[-1].clone())


class ConvGRUCell(_ConvCell):
    """The reference's ConvGRUCell (cell.py:78-136); module docstring.  `call(x, h)` returns `(h', h')`, a new tensor without `grad_fn`."""

    def __init__(self, shape, filters, kernel, activation="tanh", normalize=True, data_format="channels_last", reuse=None, differentiable=False):
        super().__init__(shape, filters, kernel, activation, normalize, data_format, differentiable)

    @property
    def state_size(self):
        return self._size

    def weight_shapes(self, in_channels):
        F, k = self._filters, self._k
        s = {"gates/kernel": (k, k, in_channels + F, 2 * F), "candidate/kernel": (k, k, in_channels + F, F)}
        if self._normalize:
            for ln in ("gates/LayerNorm", "gates/LayerNorm_1", "candidate/LayerNorm"):
                s[ln + "/gamma"] = s[ln + "/beta"] = (F,)
        else:
            s["gates/bias"] = (2 * F,)
            s["candidate/bias"] = (F,)
        return s

    def assign_weights(self, weights):
        cx = self._kernel_in_channels(weights, "gates/kernel", 2 * self._filters)
        host = {n: self._take(weights, n, s) for n, s in self.weight_shapes(cx).items()}
        if self._differentiable:
            return self._set_parameters(cx, host)
        dev = {"gates/kernel": self._padded_kernel(host["gates/kernel"], cx), "candidate/kernel": self._padded_kernel(host["candidate/kernel"], cx)}
        if self._normalize:
            dev["gates/gamma"] = np.stack([host["gates/LayerNorm/gamma"], host["gates/LayerNorm_1/gamma"]])
            dev["gates/beta"] = np.stack([host["gates/LayerNorm/beta"], host["gates/LayerNorm_1/beta"]])
            dev["candidate/gamma"] = host["candidate/LayerNorm/gamma"]
            dev["candidate/beta"] = host["candidate/LayerNorm/beta"]
        else:
            dev["gates/bias"] = host["gates/bias"]
            dev["candidate/bias"] = host["candidate/bias"]
        self._set_weights(cx, dev)

    def _dev_from(self, p):
        dev = {}
        for n in ("gates", "candidate"):
            dev[n + "/kernel"], dev[n + "/kernel4"] = self._padded_kernel_dev(p[n + "/kernel"])
        if self._normalize:
            dev["gates/gamma"] = torch.stack([p["gates/LayerNorm/gamma"], p["gates/LayerNorm_1/gamma"]])
            dev["gates/beta"] = torch.stack([p["gates/LayerNorm/beta"], p["gates/LayerNorm_1/beta"]])
            dev["candidate/gamma"] = p["candidate/LayerNorm/gamma"].contiguous()
            dev["candidate/beta"] = p["candidate/LayerNorm/beta"].contiguous()
        else:
            dev["gates/bias"] = p["gates/bias"].contiguous()
            dev["candidate/bias"] = p["candidate/bias"].contiguous()
        return dev

    def synthetic_weights(self, seed, in_channels, random_ln=False):
        """As ConvLSTMCell.synthetic_weights; the reference's initialisers: gates/bias ones, candidate/bias zeros."""
        return _synthetic(self.weight_shapes(in_channels), seed, random_ln, {"gates/bias": 1.0})

    def _make_buffers(self, B, device):
        F = self._filters
        b = _Buffers()
        b.cat = self._new_cat(B, device)
        b.cat2 = self._new_cat(B, device)
        b.y = torch.empty((B, self._H, self._W, _up4(2 * F)), dtype=torch.float32, device=device)
        b.y2 = torch.empty((B, self._H, self._W, _up4(F)), dtype=torch.float32, device=device)
        b.u = self._new_state(B, device)
        b.conv_ws = _ws(max(self._conv_ws_bytes(B, 2 * F), self._conv_ws_bytes(B, F)), device)
        b.gate_ws = _ws(_lib.lib().vstab_convgru_workspace_bytes(B, self._H, self._W, F, int(self._normalize)), device)
        return b

    def _step(self, b, h_out, between=None):
        """one step on loaded buffers: b.cat holds x and h, b.cat2 holds x; h' -> h_out and the h slice of b.cat.  between: called
        after the gates stage (the update reuses the place of its statistics)"""
        F = self._filters
        self._conv(b.cat, self._dev["gates/kernel"], self._dev.get("gates/bias"), b.y, 2 * F, b.conv_ws)
        self._gates(b)
        if between is not None:
            between()
        self._conv(b.cat2, self._dev["candidate/kernel"], self._dev.get("candidate/bias"), b.y2, F, b.conv_ws)
        self._update(b, h_out)

    def _gates(self, b):
        L, F, B, norm, st, hp = _lib.lib(), self._filters, b.cat.shape[0], int(self._normalize), runtime.stream_ptr(), self._h_slice_ptr(b.cat)
        _lib.check(L.vstab_convgru_gates(b.y.data_ptr(), b.y.shape[3], hp, self._cs, self._ptr("gates/gamma"), self._ptr("gates/beta"), B, self._H,
                                         self._W, F, norm, self._h_slice_ptr(b.cat2), self._cs, b.u.data_ptr(), b.gate_ws.data_ptr(),
                                         b.gate_ws.numel(), st))

    def _update(self, b, h_out):
        L, F, B, norm, st, hp = _lib.lib(), self._filters, b.cat.shape[0], int(self._normalize), runtime.stream_ptr(), self._h_slice_ptr(b.cat)
        _lib.check(L.vstab_convgru_update(b.y2.data_ptr(), b.y2.shape[3], hp, self._cs, b.u.data_ptr(), self._ptr("candidate/gamma"),
                                          self._ptr("candidate/beta"), B, self._H, self._W, F, self._act, norm, h_out.data_ptr(), hp, self._cs,
                                          b.gate_ws.data_ptr(), b.gate_ws.numel(), st))

    def _load_x(self, b, x):
        b.cat[..., :self._cx].copy_(x)
        b.cat2[..., :self._cx].copy_(x)

    def call(self, x, h):
        self._check_call(x, (("h", h),))
        if self._differentiable:
            self._refresh()
            if self._wants_graph(x, h):
                with torch.cuda.device(x.device):
                    h_new = _GruSequence.apply(self, x.unsqueeze(0), h, *self._params.values())[0]
                return h_new, h_new
        with torch.no_grad(), torch.cuda.device(x.device):
            b = self.buffers(x.shape[0], x.device)
            self._load_x(b, x)
            b.cat[..., self._hoff:self._hoff + self._filters].copy_(h)
            h_new = self._new_state(x.shape[0], x.device)
            self._step(b, h_new)
        return h_new, h_new

    def _sequence(self, inputs, state):
        T, B = inputs.shape[0], inputs.shape[1]
        b = self.buffers(B, inputs.device)
        outputs = torch.empty((T, B) + tuple(self._size), dtype=torch.float32, device=inputs.device)
        hs = b.cat[..., self._hoff:self._hoff + self._filters]
        if state is None:
            hs.zero_()
        else:
            hs.copy_(state)
        for t in range(T):
            self._load_x(b, inputs[t])
            self._step(b, outputs[t])
        return outputs, outputs[T - 1].clone()

    def _sequence_graph(self, inputs, state):
        h0 = torch.zeros((inputs.shape[1],) + tuple(self._size), dtype=torch.float32, device=inputs.device) if state is None else state
        outputs = _GruSequence.apply(self, inputs, h0, *self._params.values())
        return outputs, outputs[-1].clone()


# ---------------------------------------------------------------------------------------------------- differentiable mode
# One torch.autograd.Function per call / run_sequence.  The forward is the loop of `_sequence` on the same buffers (the same bits) and
# keeps, per step, a snapshot of the concat buffer(s), the convolution output(s), the old c (LSTM) / u (GRU) and the layer-norm
# statistics.  The backward walks t = T-1 .. 0: gate backward (training.conv*_backward), filter gradient (training.conv_wgrad,
# accumulating into a [k,k,cs,.] buffer in the concat layout), input gradient (training.conv_dgrad, with the kernel's output channels
# zero-padded to the gate gradient's row stride) into a concat-shaped buffer whose x slice is dx_t and whose h slice joins dh of step t-1.
def _sum_or(a, b):
    return a if b is None else a + b


def _save_steps(ctx, steps):
    """the per-step snapshots through save_for_backward (None entries remembered in ctx.layout)"""
    ctx.layout = [[t is not None for t in s] for s in steps]
    ctx.save_for_backward(*(t for s in steps for t in s if t is not None))


def _saved_steps(ctx):
    it = iter(ctx.saved_tensors)
    return [tuple(next(it) if has else None for has in s) for s in ctx.layout]


class _LstmSequence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cell, inputs, c0, h0, *params):
        T, B = inputs.shape[0], inputs.shape[1]
        H, W, F = cell._H, cell._W, cell._filters
        b = cell.buffers(B, inputs.device)
        outputs = torch.empty((T, B) + tuple(cell._size), dtype=torch.float32, device=inputs.device)
        b.cat[..., cell._hoff:cell._hoff + F].copy_(h0)
        c = c0.detach().contiguous()
        offs = [int(_lib.lib().vstab_convlstm_gates_stats_offset(B, H, W, F, q)) for q in (0, 1)] if cell._normalize else None
        steps = []
        for t in range(T):
            b.cat[..., :cell._cx].copy_(inputs[t])
            cat_t, c_new = b.cat.clone(), cell._new_state(B, inputs.device)
            cell._step(b, c, c_new, outputs[t])
            stats = (cell._stats(b.gate_ws, offs[0], 3, B), cell._stats(b.gate_ws, offs[1], 2, B)) if cell._normalize else (None, None)
            steps.append((cat_t, b.y.clone(), c) + stats)
            c = c_new
        _save_steps(ctx, steps)
        ctx.cell, ctx.dev, ctx.names = cell, cell._dev, list(cell._params)
        return outputs, c

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_c):
        cell, dev, steps = ctx.cell, ctx.dev, _saved_steps(ctx)
        T, F, cx, hoff, k, m = len(steps), cell._filters, cell._cx, cell._hoff, cell._k, 4 * cell._filters
        need_in, need_c0, need_h0 = ctx.needs_input_grad[1:4]
        need = dict(zip(ctx.names, ctx.needs_input_grad[4:]))
        need_peep = cell._peephole and any(need[n] for n in ("W_ci", "W_cf", "W_co"))
        need_ln = cell._normalize and any(v for n, v in need.items() if "LayerNorm" in n)
        need_w = need["kernel"] or need.get("bias", False)
        cat0 = steps[0][0]
        B, H, W, cs = cat0.shape
        g_out = None if g_out is None else g_out.contiguous()
        d_in = torch.empty((T, B, H, W, cx), dtype=torch.float32, device=cat0.device) if need_in else None
        dcat = torch.empty_like(cat0)
        dW = torch.empty((k, k, cs, m), dtype=torch.float32, device=cat0.device) if need_w else None
        db = torch.empty((m,), dtype=torch.float32, device=cat0.device) if need.get("bias", False) else None
        pe = tuple(dev[n] for n in ("W_ci", "W_cf", "W_co")) if cell._peephole else None
        dc, carry, pg = g_c, None, None
        for n, t in enumerate(range(T - 1, -1, -1)):
            cat_t, y, c_old = steps[t][:3]
            stats = steps[t][3:] if cell._normalize else None
            dh = carry if g_out is None else _sum_or(g_out[t], carry)
            dy, dc, pg = training.convlstm_gates_backward(y, c_old, dh, dc, pe, dev.get("gamma"), dev.get("beta"), stats, cell._forget_bias, cell._act,
                                                          need_peepholes=need_peep, need_ln=need_ln, grads=pg, accumulate=n > 0)
            if need_w:
                training.conv_wgrad(cat_t, dy, k, 1, (k - 1) // 2, cin=cs, cout=m, dW=dW, db=db, accumulate=n > 0, want_db=db is not None)
            if t > 0 or need_in or need_h0:
                training.conv_dgrad(dy, dev["kernel4"], 1, (k - 1) // 2, (H, W), cout=_up4(m), dx=dcat)
                if need_in:
                    d_in[t].copy_(dcat[..., :cx])
                carry = dcat[..., hoff:hoff + F]
        grads = {"kernel": cell._kernel_grad(dW) if need["kernel"] else None, "bias": db}
        grads.update({n: pg[n] for n in ("W_ci", "W_cf", "W_co")})
        for q, ln in enumerate(_LSTM_LN):
            for leaf in ("gamma", "beta"):
                grads[f"{ln}/{leaf}"] = pg[leaf][q] if pg[leaf] is not None else None
        return (None, d_in, dc if need_c0 else None, carry.contiguous() if need_h0 else None) + tuple(grads[n] if need[n] else None for n in ctx.names)


class _GruSequence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, cell, inputs, h0, *params):
        T, B = inputs.shape[0], inputs.shape[1]
        H, W, F = cell._H, cell._W, cell._filters
        b = cell.buffers(B, inputs.device)
        outputs = torch.empty((T, B) + tuple(cell._size), dtype=torch.float32, device=inputs.device)
        b.cat[..., cell._hoff:cell._hoff + F].copy_(h0)
        off = int(_lib.lib().vstab_convgru_stats_offset(B, H, W, F)) if cell._normalize else None
        steps = []
        for t in range(T):
            cell._load_x(b, inputs[t])
            cat_t, stats_g = b.cat.clone(), []
            cell._step(b, outputs[t], between=(lambda: stats_g.append(cell._stats(b.gate_ws, off, 2, B))) if cell._normalize else None)
            stats_c = cell._stats(b.gate_ws, off, 1, B) if cell._normalize else None
            steps.append((cat_t, b.cat2.clone(), b.y.clone(), b.y2.clone(), b.u.clone(), stats_g[0] if stats_g else None, stats_c))
        _save_steps(ctx, steps)
        ctx.cell, ctx.dev, ctx.names = cell, cell._dev, list(cell._params)
        return outputs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out):
        cell, dev, steps = ctx.cell, ctx.dev, _saved_steps(ctx)
        T, F, cx, hoff, k = len(steps), cell._filters, cell._cx, cell._hoff, cell._k
        need_in, need_h0 = ctx.needs_input_grad[1:3]
        need = dict(zip(ctx.names, ctx.needs_input_grad[3:]))
        need_ln = {p: cell._normalize and any(v for n, v in need.items() if n.startswith(p + "/LayerNorm")) for p in ("gates", "candidate")}
        need_w = {p: need[p + "/kernel"] or need.get(p + "/bias", False) for p in ("gates", "candidate")}
        cat0 = steps[0][0]
        B, H, W, cs = cat0.shape
        g_out = g_out.contiguous()
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=cat0.device)          # noqa: E731
        d_in = new(T, B, H, W, cx) if need_in else None
        dcat = torch.empty_like(cat0)
        dW = {"gates": new(k, k, cs, 2 * F) if need_w["gates"] else None, "candidate": new(k, k, cs, F) if need_w["candidate"] else None}
        db = {"gates": new(2 * F) if need.get("gates/bias", False) else None, "candidate": new(F) if need.get("candidate/bias", False) else None}
        carry, pgg, pgc, pad = None, None, None, (k - 1) // 2
        for n, t in enumerate(range(T - 1, -1, -1)):
            cat_t, cat2_t, y, y2, u, stats_g, stats_c = steps[t]
            h_old = cat_t[..., hoff:hoff + F]
            du, dy2, dh, pgc = training.convgru_update_backward(y2, h_old, u, _sum_or(g_out[t], carry), dev.get("candidate/gamma"), dev.get("candidate/beta"),
                                                                stats_c, cell._act, need_ln=need_ln["candidate"], grads=pgc, accumulate=n > 0)
            if need_w["candidate"]:
                training.conv_wgrad(cat2_t, dy2, k, 1, pad, cin=cs, cout=F, dW=dW["candidate"], db=db["candidate"], accumulate=n > 0,
                                    want_db=db["candidate"] is not None)
            training.conv_dgrad(dy2, dev["candidate/kernel4"], 1, pad, (H, W), cout=_up4(F), dx=dcat)
            drh = dcat[..., hoff:hoff + F]
            dy, pgg = training.convgru_gates_backward(y, h_old, du, drh, dh, dev.get("gates/gamma"), dev.get("gates/beta"), stats_g,
                                                      need_ln=need_ln["gates"], grads=pgg, accumulate=n > 0)
            if need_w["gates"]:
                training.conv_wgrad(cat_t, dy, k, 1, pad, cin=cs, cout=2 * F, dW=dW["gates"], db=db["gates"], accumulate=n > 0,
                                    want_db=db["gates"] is not None)
            drh.zero_()                       # (d(r h) is spent: the slice now collects the gates convolution's gradient of h)
            if t > 0 or need_in or need_h0:
                training.conv_dgrad(dy, dev["gates/kernel4"], 1, pad, (H, W), cout=_up4(2 * F), dx=dcat, accumulate=True)
                if need_in:
                    d_in[t].copy_(dcat[..., :cx])
                carry = dh + drh
        grads = {}
        for p, pg, names in (("gates", pgg, ("gates/LayerNorm", "gates/LayerNorm_1")), ("candidate", pgc, ("candidate/LayerNorm",))):
            grads[p + "/kernel"] = cell._kernel_grad(dW[p]) if need[p + "/kernel"] else None
            grads[p + "/bias"] = db[p]
            for q, ln in enumerate(names):
                for leaf in ("gamma", "beta"):
                    g = pg[leaf]
                    grads[f"{ln}/{leaf}"] = None if g is None else (g[q] if g.dim() == 2 else g)
        return (None, d_in, carry if need_h0 else None) + tuple(grads[n] if need[n] else None for n in ctx.names)


def _synthetic(shapes, seed, random_ln, constants):
    rng = np.random.RandomState(seed)
    out = {}
    for name, shape in shapes.items():
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "kernel":
            fan_in = shape[0] * shape[1] * shape[2]
            a = rng.standard_normal(shape) * np.sqrt(3.0 / fan_in)
        elif leaf in ("W_ci", "W_cf", "W_co"):
            a = rng.uniform(-0.5, 0.5, shape)
        elif leaf == "gamma":
            a = rng.uniform(0.5, 1.5, shape) if random_ln else np.ones(shape)
        elif leaf == "beta":
            a = rng.uniform(-0.5, 0.5, shape) if random_ln else np.zeros(shape)
        else:
            a = np.full(shape, constants.get(name, 0.0))
        out[name] = a.astype(np.float32)
    return out


def run_sequence(cell, inputs, state=None):
    """What tf.nn.dynamic_rnn(cell, inputs, time_major=True) gives: inputs [T,B,H,W,Cx] -> (outputs [T,B,H,W,F], final state).  The
    state, the concat buffers and the workspaces are allocated once and stay on the device across the steps (each step's h goes from
    the gate kernel straight into the concat buffer); zero state when none is given.  Bit-equal to T calls of `cell.call`."""
    if not torch.is_tensor(inputs) or not inputs.is_cuda or inputs.dtype != torch.float32 or inputs.dim() != 5 or inputs.shape[0] < 1:
        raise ValueError("inputs must be a float32 CUDA tensor [T,B,H,W,Cx]")
    if isinstance(cell, ConvLSTMCell):
        states = () if state is None else (("c", state[0]), ("h", state[1]))
    else:
        states = () if state is None else (("h", state),)
    cell._check_call(inputs[0], states)
    if cell._differentiable:
        cell._refresh()
        if cell._wants_graph(inputs, *(s for _, s in states)):
            with torch.cuda.device(inputs.device):
                return cell._sequence_graph(inputs, state)
    with torch.no_grad(), torch.cuda.device(inputs.device):
        return cell._sequence(inputs.detach(), state)
