"""Drop-in for the reference's cell.py: ConvLSTMCell (cell.py:5-76) and ConvGRUCell (cell.py:78-136) on float32 CUDA tensors in NHWC.

Forward only: results carry no `grad_fn`, whatever the inputs require (as the bicubic sampler's).  A step is the SAME convolution over
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

Not built: the backward, data_format='channels_first' (the reference passes 'NC' with feature axis 0 for it, which is wrong for a
batched tensor: NotImplementedError here), even or rectangular kernels, kernels wider than 7, and the commented-out
spatial-transformer GRU of cell.py:138-208.
"""
from __future__ import annotations

import collections

import numpy as np
import torch

from . import _lib, runtime

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


def _up4(n: int) -> int:
    return (n + 3) // 4 * 4


def _as_f32(value, name, shape):
    a = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)
    if tuple(a.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(a.shape)}, expected {tuple(shape)}")
    return np.ascontiguousarray(a, dtype=np.float32)


class _Buffers:
    """What a cell keeps on the device for one batch size."""


class _ConvCell:
    def __init__(self, shape, filters, kernel, activation, normalize, data_format):
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
                 reuse=None):
        super().__init__(shape, filters, kernel, activation, normalize, data_format)
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
        dev = {"kernel": self._padded_kernel(host["kernel"], cx)}
        for n in ("bias", "W_ci", "W_cf", "W_co"):
            if n in host:
                dev[n] = host[n]
        if self._normalize:
            dev["gamma"] = np.stack([host[ln + "/gamma"] for ln in _LSTM_LN])
            dev["beta"] = np.stack([host[ln + "/beta"] for ln in _LSTM_LN])
        self._set_weights(cx, dev)

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


class ConvGRUCell(_ConvCell):
    """The reference's ConvGRUCell (cell.py:78-136); module docstring.  `call(x, h)` returns `(h', h')`, a new tensor without `grad_fn`."""

    def __init__(self, shape, filters, kernel, activation="tanh", normalize=True, data_format="channels_last", reuse=None):
        super().__init__(shape, filters, kernel, activation, normalize, data_format)

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

    def _step(self, b, h_out):
        """one step on loaded buffers: b.cat holds x and h, b.cat2 holds x; h' -> h_out and the h slice of b.cat"""
        F = self._filters
        self._conv(b.cat, self._dev["gates/kernel"], self._dev.get("gates/bias"), b.y, 2 * F, b.conv_ws)
        self._gates(b)
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
    with torch.no_grad(), torch.cuda.device(inputs.device):
        return cell._sequence(inputs.detach(), state)
