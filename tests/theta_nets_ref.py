"""Numpy restatement of the theta regressors (reference model.py:152-184 Localizer, :375-455 dense_homo, :897-1024 flownetS_prehomo) and
of the arithmetic of each kernel under them, in the dtype of its inputs: float64 is the yardstick, float32 shows what float32 itself
costs.  Nothing here imports the package's graph tables: the three graphs are written out again from the reference, so that a slip in
theta_nets.py shows as a disagreement.  test_theta_nets_ref_cpu.py anchors every block to numpy / torch primitives."""
import numpy as np

EPS = 1e-5
SLOPE = 0.2
HOMO_SCALE = np.array([0.3, 0.1, 170, 0.1, 0.3, 170, 0.01, 0.01])
HOMO_SHIFT = np.array([1, 0, 0, 0, 1, 0, 0, 0], dtype=np.float64)


def pad_symmetric(x, p, cs=None):
    """x [B,H,W,C] -> [B,H+2p,W+2p,cs]: rows / columns mirrored with the edge sample repeated, channels C..cs-1 zero"""
    B, H, W, C = x.shape
    cs = C if cs is None else cs
    ri = [(-i - 1 if i < 0 else (2 * H - 1 - i if i >= H else i)) for i in range(-p, H + p)]
    ci = [(-j - 1 if j < 0 else (2 * W - 1 - j if j >= W else j)) for j in range(-p, W + p)]
    y = np.zeros((B, H + 2 * p, W + 2 * p, cs), x.dtype)
    y[..., :C] = x[:, ri][:, :, ci]
    return y


def lrelu(u, slope=SLOPE):
    return np.where(u >= 0, u, u.dtype.type(slope) * u)


def rstd(var, eps=EPS):
    """1 / sqrt(var + eps) in double, rounded to var's dtype (vstab_bn_lrelu_inference_forward's rule)"""
    return (1.0 / np.sqrt(var.astype(np.float64) + np.float64(np.float32(eps)))).astype(var.dtype)


def bn_lrelu(z, beta, mean, var, slope=SLOPE, twice=False, eps=EPS):
    """BatchNormLayer(act=lrelu(slope), is_train=False, no gamma) over the last axis; `twice`: lrelu on the input as well"""
    t = lrelu(z, slope) if twice else z
    return lrelu((t - mean) * rstd(var, eps) + beta, slope)


def maxpool_same(y):
    """2x2 stride-2 SAME max pool of [B,H,W,C], the window clipped at an odd edge"""
    B, H, W, C = y.shape
    out = np.empty((B, (H + 1) // 2, (W + 1) // 2, C), y.dtype)
    for i in range(out.shape[1]):
        for j in range(out.shape[2]):
            out[:, i, j] = y[:, 2 * i:2 * i + 2, 2 * j:2 * j + 2].max(axis=(1, 2))
    return out


def conv3x3_valid(x, W, b, stride=1):
    """x [B,H,W,Cin], W [3,3,Cin,Cout] (HWIO), b [Cout] -> [B,(H-3)//s+1,(W-3)//s+1,Cout]"""
    B, H, Wd, _ = x.shape
    ho, wo = (H - 3) // stride + 1, (Wd - 3) // stride + 1
    out = np.zeros((B, ho, wo, W.shape[3]), x.dtype)
    for di in range(3):
        for dj in range(3):
            patch = x[:, di:di + (ho - 1) * stride + 1:stride, dj:dj + (wo - 1) * stride + 1:stride]
            out += patch @ W[di, dj]
    return out + b


def dense(x, W, b, act="identity", slope=SLOPE):
    u = x @ W + b
    if act == "identity":
        return u
    if act == "lrelu":
        return lrelu(u, slope)
    if act == "tanh":
        return np.tanh(u)
    if act == "tanh_affine":
        return np.tanh(u / u.dtype.type(1000)) * HOMO_SCALE.astype(u.dtype) + HOMO_SHIFT.astype(u.dtype)
    raise ValueError(act)


def _cast(w, dtype):
    return {k: np.asarray(v).astype(dtype) for k, v in w.items()}


def _conv_bn(x, w, conv, bn, stride=1, pad=1):
    if pad:
        x = pad_symmetric(x, pad)
    z = conv3x3_valid(x, w[f"{conv}/W_conv2d"], w[f"{conv}/b_conv2d"], stride)
    return bn_lrelu(z, w[f"{bn}/beta"], w[f"{bn}/moving_mean"], w[f"{bn}/moving_variance"])


def _dense_bn(x, w, name, bn, act):
    y = dense(x, w[f"{name}/W"], w[f"{name}/b"], act)
    return bn_lrelu(y, w[f"{bn}/beta"], w[f"{bn}/moving_mean"], w[f"{bn}/moving_variance"])


def localizer(feats, w, is_tanh=False, dtype=np.float64):
    """model.py:152-184"""
    w, n = _cast(w, dtype), np.asarray(feats).astype(dtype)
    n = _conv_bn(n, w, "d1/c1", "d1/b1", stride=2, pad=0)
    for d in ("d2", "d3", "d4", "d5"):
        n = _conv_bn(n, w, f"{d}/c1", f"{d}/b1", pad=0)
    n = n.reshape(n.shape[0], -1)                                  # FlattenLayer: NHWC order
    n = _dense_bn(n, w, "df/dense1", "df/b1", "identity")
    return dense(n, w["df/dense2/W"], w["df/dense2/b"], "tanh" if is_tanh else "identity")


def flownets_prehomo(feats, w, dtype=np.float64):
    """model.py:897-959 (and :962-1024)"""
    w, n = _cast(w, dtype), np.asarray(feats).astype(dtype)
    for blk in (1, 2, 3, 4):
        for i in (1, 2, 3):
            n = _conv_bn(n, w, f"conv{blk}_{i}", f"bn{blk}_{i}")
        n = maxpool_same(n)
    n = n.reshape(n.shape[0], -1)
    n = _dense_bn(n, w, "df/dense1", "df/b1", "lrelu")
    n = _dense_bn(n, w, "df/dense2", "df/b2", "lrelu")
    return dense(n, w["df/dense3/W"], w["df/dense3/b"])


def dense_homo(feats, w, dtype=np.float64, literal=False):
    """model.py:375-455.  `literal=True` also evaluates the layers whose outputs the reference drops (each reads net_in), as the
    reference's graph construction does, and needs their variables."""
    w, net_in = _cast(w, dtype), np.asarray(feats).astype(dtype)
    n = None
    if literal:
        for name in ("1_1", "1_2", "1_3"):
            n = _conv_bn(net_in, w, f"conv{name}", f"bn{name}")
        n = maxpool_same(n)
        for name in ("2_1", "2_2"):
            n = _conv_bn(net_in, w, f"conv{name}", f"bn{name}")
    n = _conv_bn(net_in, w, "conv2_3", "bn2_3")
    n = maxpool_same(n)
    n = n.reshape(n.shape[0], -1)
    n = _dense_bn(n, w, "df/dense1", "df/b1", "lrelu")
    n = _dense_bn(n, w, "df/dense2", "df/b2", "lrelu")
    n = dense(n, w["df/dense3/W"], w["df/dense3/b"], "tanh_affine")
    n = np.concatenate([n, np.ones((n.shape[0], 1), n.dtype)], axis=1)          # model.py:422-427
    return n.reshape(-1, 3, 3).reshape(-1, 9)[:, 0:8]


FORWARD = {"Localizer": localizer, "flownetS_prehomo": flownets_prehomo, "flownetS_variableWeight": flownets_prehomo,
           "dense_homo": dense_homo}


def bound_ratio(got, w, feats, net, **kw):
    """(err(got) / max|ref64|, err(fp32 restatement) / max|ref64|) against the float64 restatement on the same inputs and weights"""
    ref = FORWARD[net](feats, w, dtype=np.float64, **kw)
    f32 = FORWARD[net](feats, w, dtype=np.float32, **kw)
    mag = np.abs(ref).max()
    return np.abs(np.asarray(got, np.float64) - ref).max() / mag, np.abs(f32.astype(np.float64) - ref).max() / mag
