"""Plain numpy restatement of the BACKWARD of the recurrent cells: analytic adjoints of `conv_same`, `layer_norm`, the gate stages, one
cell step and back-propagation through time over `run_sequence`, parameterised by dtype like tests/cell_ref.py (every array is cast to
`dtype` first and every operation runs in it).  The forward pieces are cell_ref's, imported, not copied.  No torch.  Pinned by
tests/test_cell_grad_ref_cpu.py against torch.autograd in float64; the GPU tests (tests/test_gpu_cell_backward.py) compare against the
float64 form and take their bounds from the float32 form's distance to it.

Adjoints, with dX the gradient of the loss with respect to X:
  conv      dx[b,i,j,c] = sum_{a,b',n} dy[b, i-a+p, j-b'+p, n] W[a,b',c,n];  dW[a,b',c,n] = sum_{b,i,j} x[b, i+a-p, j+b'-p, c] dy[b,i,j,n]
  layer norm  xhat = (v - mean) rstd, g = dout gamma:  dv = rstd (g - mean_N(g) - xhat mean_N(g xhat)),
            dgamma[c] = sum_{b,i,j} dout xhat,  dbeta[c] = sum_{b,i,j} dout
  sigmoid'  s (1 - s);  tanh' 1 - tanh^2;  relu' (v > 0);  identity' 1
  LSTM / GRU: the chain rule through cell_ref.lstm_gates / gru_gates / gru_update in reverse order (see the functions).
Parameter gradients come back as a dict with the names and shapes of the weights.
"""
import functools

import numpy as np

from tests import cell_ref as ref
from tests.cell_ref import GRU_LN, LSTM_LN


# ---------------------------------------------------------------------------------------------------- pieces
def conv_same_adjoint(x, w, dy):
    """(dx, dw) of y = cell_ref.conv_same(x, w)"""
    B, H, W, C = x.shape
    k = w.shape[0]
    p = (k - 1) // 2
    xp = np.zeros((B, H + 2 * p, W + 2 * p, C), x.dtype)
    xp[:, p:p + H, p:p + W] = x
    dxp = np.zeros_like(xp)
    dw = np.zeros_like(w)
    for a in range(k):
        for b in range(k):
            for c in range(C):
                dxp[:, a:a + H, b:b + W, c] += (dy * w[a, b, c]).sum(axis=3, dtype=x.dtype)
                dw[a, b, c] = (xp[:, a:a + H, b:b + W, c:c + 1] * dy).sum(axis=(0, 1, 2), dtype=x.dtype)
    return dxp[:, p:p + H, p:p + W], dw


def layer_norm_adjoint(v, gamma, dout):
    """(dv, dgamma, dbeta) of cell_ref.layer_norm(v, gamma, beta)"""
    dt = v.dtype
    mean = v.mean(axis=(1, 2, 3), keepdims=True, dtype=dt)
    d = v - mean
    var = (d * d).mean(axis=(1, 2, 3), keepdims=True, dtype=dt)
    rstd = dt.type(1) / np.sqrt(var + dt.type(1e-12))
    xhat = d * rstd
    g = dout * gamma
    dv = rstd * (g - g.mean(axis=(1, 2, 3), keepdims=True, dtype=dt) - xhat * (g * xhat).mean(axis=(1, 2, 3), keepdims=True, dtype=dt))
    return dv, (dout * xhat).sum(axis=(0, 1, 2), dtype=dt), dout.sum(axis=(0, 1, 2), dtype=dt)


def act_grad(v, activation):
    if activation == "tanh":
        t = np.tanh(v)
        return v.dtype.type(1) - t * t
    if activation == "relu":
        return (v > 0).astype(v.dtype)
    assert activation == "identity"
    return np.ones_like(v)


def _ln_back(v, w, name, dout, grads):
    dv, grads[name + "/gamma"], grads[name + "/beta"] = layer_norm_adjoint(v, w[name + "/gamma"], dout)
    return dv


def _zero(like, d):
    return np.zeros_like(like) if d is None else np.asarray(d, like.dtype)


# ---------------------------------------------------------------------------------------------------- gate stages
def lstm_gates_backward(y, c, w, dh, dc_new, forget_bias=1.0, activation="tanh", normalize=True, peephole=True):
    """adjoint of cell_ref.lstm_gates (everything in y's dtype; w cast already): returns (dy, dc, grads).  dh / dc_new None = zero"""
    F = c.shape[3]
    one = y.dtype.type(1)
    # forward, keeping what the adjoint needs
    j, i, f, o = (y[..., g * F:(g + 1) * F] for g in range(4))
    if peephole:
        i = i + w["W_ci"] * c
        f = f + w["W_cf"] * c
    j_raw, i_raw, f_raw = j, i, f
    if normalize:
        j, i, f = (ref.layer_norm(v, w[LSTM_LN[n] + "/gamma"], w[LSTM_LN[n] + "/beta"]) for n, v in enumerate((j, i, f)))
    fs, is_, aj = ref.sigmoid(f + y.dtype.type(forget_bias)), ref.sigmoid(i), ref.act(j, activation)
    c_raw = c * fs + is_ * aj
    if peephole:
        o = o + w["W_co"] * c_raw
    o_raw, cn = o, c_raw
    if normalize:
        o, cn = ref.layer_norm(o_raw, w[LSTM_LN[3] + "/gamma"], w[LSTM_LN[3] + "/beta"]), ref.layer_norm(c_raw, w[LSTM_LN[4] + "/gamma"], w[LSTM_LN[4] + "/beta"])
    so, ac = ref.sigmoid(o), ref.act(cn, activation)
    # backward
    grads = {}
    dh, dcn = _zero(c, dh), _zero(c, dc_new)
    d_o = dh * ac * so * (one - so)
    d_c = dcn + dh * so * act_grad(cn, activation)
    if normalize:
        d_o = _ln_back(o_raw, w, LSTM_LN[3], d_o, grads)
        d_c = _ln_back(c_raw, w, LSTM_LN[4], d_c, grads)
    if peephole:
        d_c = d_c + w["W_co"] * d_o
        grads["W_co"] = (d_o * c_raw).sum(axis=0, dtype=y.dtype)
    d_f = d_c * c * fs * (one - fs)
    d_i = d_c * aj * is_ * (one - is_)
    d_j = d_c * is_ * act_grad(j, activation)
    dc = d_c * fs
    if normalize:
        d_j, d_i, d_f = (_ln_back(v, w, LSTM_LN[n], d, grads) for n, (v, d) in enumerate(((j_raw, d_j), (i_raw, d_i), (f_raw, d_f))))
    if peephole:
        dc = dc + w["W_ci"] * d_i + w["W_cf"] * d_f
        grads["W_ci"] = (d_i * c).sum(axis=0, dtype=y.dtype)
        grads["W_cf"] = (d_f * c).sum(axis=0, dtype=y.dtype)
    return np.concatenate([d_j, d_i, d_f, d_o], axis=3), dc, grads


def gru_update_backward(y2, h, u, w, dhn, activation="tanh", normalize=True):
    """adjoint of cell_ref.gru_update: returns (du, dy2, dh, grads) with dh = dhn u (the direct path only)"""
    grads = {}
    y2n = ref.layer_norm(y2, w[GRU_LN[2] + "/gamma"], w[GRU_LN[2] + "/beta"]) if normalize else y2
    du = dhn * (h - ref.act(y2n, activation))
    dy2 = dhn * (y2.dtype.type(1) - u) * act_grad(y2n, activation)
    if normalize:
        dy2 = _ln_back(y2, w, GRU_LN[2], dy2, grads)
    return du, dy2, dhn * u, grads


def gru_gates_backward(y, h, w, du, drh, normalize=True):
    """adjoint of cell_ref.gru_gates: returns (dy = [dr, du], dh = drh r, grads)"""
    F = h.shape[3]
    one = y.dtype.type(1)
    grads = {}
    r_raw, u_raw = y[..., :F], y[..., F:2 * F]
    r, u = r_raw, u_raw
    if normalize:
        r, u = (ref.layer_norm(v, w[GRU_LN[n] + "/gamma"], w[GRU_LN[n] + "/beta"]) for n, v in enumerate((r, u)))
    r, u = ref.sigmoid(r), ref.sigmoid(u)
    d_r = drh * h * r * (one - r)
    d_u = du * u * (one - u)
    if normalize:
        d_r, d_u = _ln_back(r_raw, w, GRU_LN[0], d_r, grads), _ln_back(u_raw, w, GRU_LN[1], d_u, grads)
    return np.concatenate([d_r, d_u], axis=3), drh * r, grads


# ---------------------------------------------------------------------------------------------------- one step
def lstm_call_backward(x, state, w, dtype, dh, dc_new, forget_bias=1.0, activation="tanh", normalize=True, peephole=True):
    """adjoint of cell_ref.lstm_call: returns (dx, (dc, dh_old), grads)"""
    w = ref.cast(w, dtype)
    x, c, h = (np.asarray(a, dtype=dtype) for a in (x, state[0], state[1]))
    cat = np.concatenate([x, h], axis=3)
    y = ref.conv_same(cat, w["kernel"])
    if not normalize:
        y = y + w["bias"]
    dy, dc, grads = lstm_gates_backward(y, c, w, dh, dc_new, forget_bias, activation, normalize, peephole)
    if not normalize:
        grads["bias"] = dy.sum(axis=(0, 1, 2), dtype=dtype)
    dcat, grads["kernel"] = conv_same_adjoint(cat, w["kernel"], dy)
    Cx = x.shape[3]
    return dcat[..., :Cx], (dc, dcat[..., Cx:]), grads


def gru_call_backward(x, h, w, dtype, dhn, activation="tanh", normalize=True):
    """adjoint of cell_ref.gru_call: returns (dx, dh_old, grads)"""
    w = ref.cast(w, dtype)
    x, h, dhn = (np.asarray(a, dtype=dtype) for a in (x, h, dhn))
    Cx = x.shape[3]
    cat = np.concatenate([x, h], axis=3)
    y = ref.conv_same(cat, w["gates/kernel"])
    if not normalize:
        y = y + w["gates/bias"]
    rh, u = ref.gru_gates(y, h, w, normalize)
    cat2 = np.concatenate([x, rh], axis=3)
    y2 = ref.conv_same(cat2, w["candidate/kernel"])
    if not normalize:
        y2 = y2 + w["candidate/bias"]
    du, dy2, dh, grads = gru_update_backward(y2, h, u, w, dhn, activation, normalize)
    if not normalize:
        grads["candidate/bias"] = dy2.sum(axis=(0, 1, 2), dtype=dtype)
    dcat2, grads["candidate/kernel"] = conv_same_adjoint(cat2, w["candidate/kernel"], dy2)
    dy, dh_r, g2 = gru_gates_backward(y, h, w, du, dcat2[..., Cx:], normalize)
    grads.update(g2)
    if not normalize:
        grads["gates/bias"] = dy.sum(axis=(0, 1, 2), dtype=dtype)
    dcat, grads["gates/kernel"] = conv_same_adjoint(cat, w["gates/kernel"], dy)
    return dcat2[..., :Cx] + dcat[..., :Cx], dh + dh_r + dcat[..., Cx:], grads


# ---------------------------------------------------------------------------------------------------- BPTT
def run_sequence_backward(kind, inputs, state, w, dtype, d_outputs, d_final, **kw):
    """adjoint of cell_ref.run_sequence: d_outputs [T,B,H,W,F], d_final the gradient of the final state ((dc, dh) for the LSTM, None
    entries = zero).  Returns (d_inputs, d_state, grads); parameter gradients are summed from t = T-1 down to 0."""
    T, B, H, W, _ = inputs.shape
    F = w["kernel" if kind == "lstm" else "candidate/kernel"].shape[3] // (4 if kind == "lstm" else 1)
    if state is None:
        z = np.zeros((B, H, W, F), dtype)
        state = (z, z) if kind == "lstm" else z
    states = [state]
    for t in range(T):
        _, s = (ref.lstm_call if kind == "lstm" else ref.gru_call)(inputs[t], states[-1], w, dtype, **kw)
        states.append(s)
    d_outputs = np.asarray(d_outputs, dtype)
    z = np.zeros((B, H, W, F), dtype)
    if kind == "lstm":
        dc, dh = _zero(z, d_final[0]), _zero(z, d_final[1])
    else:
        dh = _zero(z, d_final)
    d_inputs, total = [None] * T, None
    for t in range(T - 1, -1, -1):
        if kind == "lstm":
            d_inputs[t], (dc, dh), grads = lstm_call_backward(inputs[t], states[t], w, dtype, dh + d_outputs[t], dc, **kw)
        else:
            d_inputs[t], dh, grads = gru_call_backward(inputs[t], states[t], w, dtype, dh + d_outputs[t], **kw)
        total = grads if total is None else {n: total[n] + grads[n] for n in grads}
    return np.stack(d_inputs), ((dc, dh) if kind == "lstm" else dh), total


# ---------------------------------------------------------------------------------------------------- cases of the GPU tests
# (also read by tests/test_cell_grad_ref_cpu.py, which asserts the conditioning the GPU bounds rely on.)  Inputs as test_gpu_cell.py
# makes them, with seeds of their own; upstream gradients N(0,1).
def _seed(shape, *flags):
    return 7000 + 41 * shape[1] + 13 * shape[4] + sum(1 << n for n, f in enumerate(flags) if f)


def _normal(seed, *shape):
    return np.random.RandomState(seed).standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def lstm_case(shape, normalize, peephole):
    """(w, x, c, h, dh, dc_new)"""
    s = _seed(shape, normalize, peephole)
    B, H, W, _, F, _ = shape
    return (ref.make_weights("lstm", s, shape, normalize, peephole),) + ref.make_inputs(s + 1, shape) + (_normal(s + 2, B, H, W, F), _normal(s + 3, B, H, W, F))


@functools.lru_cache(maxsize=None)
def gru_case(shape, normalize):
    """(w, x, h, dh_new, du, drh): du and drh feed the gates stage alone"""
    s = _seed(shape, normalize) + 500
    B, H, W, _, F, _ = shape
    x, _, h = ref.make_inputs(s + 1, shape)
    return (ref.make_weights("gru", s, shape, normalize), x, h) + tuple(_normal(s + 2 + n, B, H, W, F) for n in range(3))


@functools.lru_cache(maxsize=None)
def stage_y(shape, gates):
    return ref.make_y(9000 + shape[1] + gates, shape, gates)


@functools.lru_cache(maxsize=None)
def stage_u(shape):
    """an update gate for the update stage alone, in (0, 1)"""
    B, H, W, _, F, _ = shape
    return np.random.RandomState(9100 + shape[1]).uniform(0.05, 0.95, (B, H, W, F)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def sequence_case(kind):
    """(w, inputs [3,...], c0, h0, d_outputs, d_final_c, d_final_h) on `odd`"""
    shape = ref.SHAPES["odd"]
    B, H, W, _, F, _ = shape
    x, c, h = ref.make_inputs(9201, shape, T=3)
    return (ref.make_weights(kind, 9200, shape, True), x, c, h, _normal(9202, 3, B, H, W, F), _normal(9203, B, H, W, F), _normal(9204, B, H, W, F))
