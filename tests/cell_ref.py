"""Plain numpy restatement of the recurrent cells (ConvLSTMCell, ConvGRUCell), their layer norm and run_sequence, parameterised by
dtype: every array is cast to `dtype` first and every operation runs in it.  No torch.  Pinned by tests/test_cell_ref_cpu.py; the
GPU tests (tests/test_gpu_cell.py) compare against the float64 form and take their bounds from the float32 form's distance to it.

In index form, with SAME zero padding p = (k-1)/2, F = filters, N = H*W*F:
  conv      y[b,i,j,n] = sum_{a,b',c} x[b, i+a-p, j+b'-p, c] W[a,b',c,n]
  layer norm (warning: recalled from TensorFlow 1.10's tf.contrib.layers.layer_norm, defaults; stated in layer_norm() only)
            mean_b = (1/N) sum_{i,j,c} v[b,i,j,c],  var_b = (1/N) sum (v - mean_b)^2,
            out[b,i,j,c] = (v[b,i,j,c] - mean_b) * (1 / sqrt(var_b + 1e-12)) * gamma[c] + beta[c]
  LSTM      y = conv(concat(x, h), kernel) (+ bias unless normalize);  j, i, f, o = y[..., 0:F], [F:2F], [2F:3F], [3F:4F]
            peephole: i += W_ci c, f += W_cf c;  normalize: j, i, f = LN_0, LN_1, LN_2
            f = sigmoid(f + forget_bias), i = sigmoid(i), c' = c f + i act(j)
            peephole: o += W_co c';  normalize: o = LN_3(o), c' = LN_4(c');  h' = sigmoid(o) act(c')
  GRU       y = conv(concat(x, h), gates/kernel);  normalize: r, u = LN_0(y[..., 0:F]), LN_1(y[..., F:2F]), else y + gates/bias
            r, u = sigmoid;  y2 = conv(concat(x, r h), candidate/kernel);  normalize: LN(y2), else + candidate/bias
            h' = u h + (1 - u) act(y2)
filters == 1 is the same formulas.
"""
import numpy as np

LSTM_LN = ("LayerNorm", "LayerNorm_1", "LayerNorm_2", "LayerNorm_3", "LayerNorm_4")          # call order j, i, f, o, c
GRU_LN = ("gates/LayerNorm", "gates/LayerNorm_1", "candidate/LayerNorm")                      # r, u, candidate

# the GPU test cases: B, H, W, Cx, F, k
SHAPES = {"f1": (1, 5, 7, 3, 1, 3), "odd": (2, 6, 10, 5, 6, 3), "k5": (3, 9, 13, 4, 8, 5), "big": (2, 24, 40, 8, 32, 3)}


def conv_same(x, w):
    B, H, W, _ = x.shape
    k = w.shape[0]
    p = (k - 1) // 2
    xp = np.zeros((B, H + 2 * p, W + 2 * p, x.shape[3]), x.dtype)
    xp[:, p:p + H, p:p + W] = x
    y = np.zeros((B, H, W, w.shape[3]), x.dtype)
    for a in range(k):                      # one product and one addition per (a, b', c), in this order and in x's dtype: the plain
        for b in range(k):                  # index sum, independent of how a BLAS would block it
            for c in range(x.shape[3]):
                y += xp[:, a:a + H, b:b + W, c:c + 1] * w[a, b, c]
    return y


def layer_norm(v, gamma, beta):
    dt = v.dtype
    mean = v.mean(axis=(1, 2, 3), keepdims=True, dtype=dt)
    d = v - mean
    var = (d * d).mean(axis=(1, 2, 3), keepdims=True, dtype=dt)
    return d * (dt.type(1) / np.sqrt(var + dt.type(1e-12))) * gamma + beta


def sigmoid(v):
    return v.dtype.type(1) / (v.dtype.type(1) + np.exp(-v))


def act(v, activation):
    if activation == "tanh":
        return np.tanh(v)
    if activation == "relu":
        return np.maximum(v, v.dtype.type(0))
    assert activation == "identity"
    return v


def cast(weights, dtype):
    return {n: np.asarray(a, dtype=dtype) for n, a in weights.items()}


def lstm_gates(y, c, w, forget_bias=1.0, activation="tanh", normalize=True, peephole=True, peephole_wrong=None, trace=None):
    """everything after the convolution (and its bias): returns (c', h').  trace: a list that receives every quantity a layer norm
    is applied to.  peephole_wrong: 'new_for_if' / 'old_for_o' build the two wrong variants the tests tell apart."""
    F = c.shape[3]
    j, i, f, o = (y[..., g * F:(g + 1) * F] for g in range(4))
    ln = lambda v, n: _ln(v, w, LSTM_LN[n], trace)                    # noqa: E731
    if peephole and peephole_wrong != "new_for_if":
        i = i + w["W_ci"] * c
        f = f + w["W_cf"] * c
    if normalize:
        j, i, f = ln(j, 0), ln(i, 1), ln(f, 2)
    f = sigmoid(f + y.dtype.type(forget_bias))
    i = sigmoid(i)
    cn = c * f + i * act(j, activation)
    if peephole_wrong == "new_for_if":                                   # (what using c' for i and f would give: one fixed-point step)
        i2 = y[..., F:2 * F] + w["W_ci"] * cn
        f2 = y[..., 2 * F:3 * F] + w["W_cf"] * cn
        cn = c * sigmoid(f2 + y.dtype.type(forget_bias)) + sigmoid(i2) * act(y[..., :F], activation)
    if peephole:
        o = o + w["W_co"] * (c if peephole_wrong == "old_for_o" else cn)
    if normalize:
        o, cn = ln(o, 3), ln(cn, 4)
    return cn, sigmoid(o) * act(cn, activation)


def _ln(v, w, name, trace):
    if trace is not None:
        trace.append(v)
    return layer_norm(v, w[name + "/gamma"], w[name + "/beta"])


def lstm_call(x, state, w, dtype, forget_bias=1.0, activation="tanh", normalize=True, peephole=True, trace=None):
    """returns (h', (c', h'))"""
    w = cast(w, dtype)
    x, c, h = (np.asarray(a, dtype=dtype) for a in (x, state[0], state[1]))
    y = conv_same(np.concatenate([x, h], axis=3), w["kernel"])
    if not normalize:
        y = y + w["bias"]
    cn, hn = lstm_gates(y, c, w, forget_bias, activation, normalize, peephole, trace=trace)
    return hn, (cn, hn)


def gru_gates(y, h, w, normalize=True, trace=None):
    """r h and u from the gates' convolution output (bias added already when not normalize)"""
    F = h.shape[3]
    r, u = y[..., :F], y[..., F:2 * F]
    if normalize:
        r, u = _ln(r, w, GRU_LN[0], trace), _ln(u, w, GRU_LN[1], trace)
    return sigmoid(r) * h, sigmoid(u)


def gru_update(y2, h, u, w, activation="tanh", normalize=True, trace=None):
    if normalize:
        y2 = _ln(y2, w, GRU_LN[2], trace)
    return u * h + (y2.dtype.type(1) - u) * act(y2, activation)


def gru_call(x, h, w, dtype, activation="tanh", normalize=True, trace=None):
    """returns (h', h')"""
    w = cast(w, dtype)
    x, h = np.asarray(x, dtype=dtype), np.asarray(h, dtype=dtype)
    y = conv_same(np.concatenate([x, h], axis=3), w["gates/kernel"])
    if not normalize:
        y = y + w["gates/bias"]
    rh, u = gru_gates(y, h, w, normalize, trace)
    y2 = conv_same(np.concatenate([x, rh], axis=3), w["candidate/kernel"])
    if not normalize:
        y2 = y2 + w["candidate/bias"]
    hn = gru_update(y2, h, u, w, activation, normalize, trace)
    return hn, hn


def run_sequence(kind, inputs, state, w, dtype, **kw):
    """tf.nn.dynamic_rnn(time_major=True): inputs [T,B,H,W,Cx] -> (outputs [T,B,H,W,F], final state); zero state when None"""
    T, B, H, W, _ = inputs.shape
    F = w["kernel" if kind == "lstm" else "candidate/kernel"].shape[3] // (4 if kind == "lstm" else 1)
    if state is None:
        z = np.zeros((B, H, W, F), dtype)
        state = (z, z) if kind == "lstm" else z
    outs = []
    for t in range(T):
        out, state = (lstm_call if kind == "lstm" else gru_call)(inputs[t], state, w, dtype, **kw)
        outs.append(out)
    return np.stack(outs), state


# ---------------------------------------------------------------------------------------------------- inputs of the GPU tests
def weight_shapes(kind, H, W, Cx, F, k, normalize, peephole=True):
    if kind == "lstm":
        s = {"kernel": (k, k, Cx + F, 4 * F)}
        if not normalize:
            s["bias"] = (4 * F,)
        if peephole:
            s.update({n: (H, W, F) for n in ("W_ci", "W_cf", "W_co")})
        ln = LSTM_LN if normalize else ()
    else:
        s = {"gates/kernel": (k, k, Cx + F, 2 * F), "candidate/kernel": (k, k, Cx + F, F)}
        if not normalize:
            s["gates/bias"] = (2 * F,)
            s["candidate/bias"] = (F,)
        ln = GRU_LN if normalize else ()
    for n in ln:
        s[n + "/gamma"] = s[n + "/beta"] = (F,)
    return s


def make_weights(kind, seed, shape, normalize, peephole=True):
    """float32 weights with every tensor random: kernels N(0, 3 / fan_in) so that pre-activations of U(-1,1) inputs are O(1),
    peepholes and biases U(-0.5, 0.5), gamma U(0.5, 1.5), beta U(-0.5, 0.5)"""
    _, H, W, Cx, F, k = shape
    rng = np.random.RandomState(seed)
    out = {}
    for name, s in weight_shapes(kind, H, W, Cx, F, k, normalize, peephole).items():
        leaf = name.rsplit("/", 1)[-1]
        if leaf == "kernel":
            a = rng.standard_normal(s) * np.sqrt(3.0 / (s[0] * s[1] * s[2]))
        elif leaf == "gamma":
            a = rng.uniform(0.5, 1.5, s)
        else:
            a = rng.uniform(-0.5, 0.5, s)
        out[name] = a.astype(np.float32)
    return out


def make_inputs(seed, shape, T=None):
    """x (or [T] of them) and a state pair, U(-1,1), float32"""
    B, H, W, Cx, F, _ = shape
    rng = np.random.RandomState(seed)
    x = rng.uniform(-1, 1, ((T,) if T else ()) + (B, H, W, Cx)).astype(np.float32)
    c = rng.uniform(-1, 1, (B, H, W, F)).astype(np.float32)
    h = rng.uniform(-1, 1, (B, H, W, F)).astype(np.float32)
    return x, c, h


def make_y(seed, shape, gates):
    """a convolution output for the post-convolution tests: N(0,1), float32, [B,H,W,gates*F]"""
    B, H, W, _, F, _ = shape
    return np.random.RandomState(seed).standard_normal((B, H, W, gates * F)).astype(np.float32)


def max_err(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))
