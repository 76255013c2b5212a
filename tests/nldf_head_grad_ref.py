"""Float64 numpy reference of the NLDF head's backward (NLDF.Model.backward), stage by stage and as the
whole walk, parametric in fea_dim, the pool sizes and the pool channel counts.

Once the activations are fixed the backward is a linear map, so every function takes the saved activations and gates on
`activation > 0`; none runs a forward of its own.  A ReLU that flips between float32 and float64 therefore cannot enter a
comparison.  `torch_forward` (the head in torch, any dtype) supplies activations and the autograd truth for the CPU tests;
`torch_walk` is the same walk as `walk` built from torch's own per-layer vector-Jacobian products, the float32 yardstick of the GPU
tests.  Tensors are NHWC; W of a convolution is HWIO, of a transposed convolution [5,5,out,in] as in the reference."""
import numpy as np
import torch
import torch.nn.functional as F

LAYERS = ("Fea_Global_1", "Fea_Global_2", "Fea_Global", "Fea_P1", "Fea_P2", "Fea_P3", "Fea_P4", "Fea_P5", "Fea_P5_Deconv", "Fea_P4_Deconv",
          "Fea_P3_Deconv", "Fea_P2_Deconv", "Local_Fea", "Local_Score", "Global_Score")


def synthetic_weights(fea, pool_c, seed=3, scale=0.3):
    """Head variables at fea_dim = fea and pool channels pool_c, in NLDF.HEAD_SHAPES' layouts."""
    rng = np.random.default_rng(seed)
    shapes = {"Fea_Global_1": (5, 5, pool_c[4], fea), "Fea_Global_2": (5, 5, fea, fea), "Fea_Global": (3, 3, fea, fea)}
    shapes.update({f"Fea_P{k + 1}": (3, 3, pool_c[k], fea) for k in range(5)})
    shapes.update({f"Fea_P{k}_Deconv": (5, 5, (6 - k) * fea, (7 - k) * fea) for k in (5, 4, 3, 2)})
    shapes.update({"Local_Fea": (1, 1, 6 * fea, 5 * fea), "Local_Score": (1, 1, 5 * fea, 2), "Global_Score": (1, 1, fea, 2)})
    out = {}
    for name in LAYERS:
        shp = shapes[name]
        fan = shp[0] * shp[1] * (shp[3] if "Deconv" in name else shp[2])
        out[name + "/W"] = rng.standard_normal(shp) * scale / np.sqrt(fan) * 3.0
        out[name + "/b"] = rng.standard_normal(shp[2] if "Deconv" in name else shp[3]) * 0.05
    return out


# ----------------------------------------------------------------------------- stages (numpy, float64)
def relu_gate(act, g):
    return np.where(act > 0, g, 0.0)


def conv_dgrad(g, W, pad, hw_in):
    """Input gradient of a stride-1 k x k convolution with `pad` zeros on every side: g [B,Ho,Wo,Co], W [k,k,Ci,Co] -> [B,hw_in,hw_in,Ci]."""
    k = W.shape[0]
    B, Ho, Wo, _ = g.shape
    dx = np.zeros((B, hw_in + 2 * pad, hw_in + 2 * pad, W.shape[2]))
    for ky in range(k):
        for kx in range(k):
            dx[:, ky:ky + Ho, kx:kx + Wo] += g @ W[ky, kx].T
    return dx[:, pad:pad + hw_in, pad:pad + hw_in]


def conv_wgrad(x, g, k, pad):
    """Filter and bias gradient of the same convolution: x [B,H,W,Ci], g [B,Ho,Wo,Co] -> dW [k,k,Ci,Co], db [Co]."""
    B, Ho, Wo, Co = g.shape
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    g2 = g.reshape(-1, Co)
    dW = np.empty((k, k, x.shape[3], Co))
    for ky in range(k):
        for kx in range(k):
            dW[ky, kx] = np.ascontiguousarray(xp[:, ky:ky + Ho, kx:kx + Wo]).reshape(-1, x.shape[3]).T @ g2
    return dW, g2.sum(0)


def deconv_backward(dup, x, W):
    """5x5 stride-2 SAME transposed convolution x [B,h,h,Cin] -> up [B,2h,2h,Cout] with W [5,5,Cout,Cin]: input (i, j) adds tap (ky, kx) at
    output (2i+ky-1, 2j+kx-1).  dup: the gradient at its pre-activation.  Returns (dx, dW, db): dx is the plain stride-2 convolution of
    dup (one row / column of padding before, two after) with W read as HWIO."""
    B, h, _, Cin = x.shape
    Cout = dup.shape[3]
    gp = np.pad(dup, ((0, 0), (1, 2), (1, 2), (0, 0)))
    dx = np.zeros((B, h, h, Cin))
    dW = np.empty((5, 5, Cout, Cin))
    x2 = x.reshape(-1, Cin)
    for ky in range(5):
        for kx in range(5):
            s = np.ascontiguousarray(gp[:, ky:ky + 2 * h:2, kx:kx + 2 * h:2]).reshape(-1, Cout)
            dx += (s @ W[ky, kx]).reshape(B, h, h, Cin)
            dW[ky, kx] = s.T @ x2
    return dx, dW, dup.reshape(-1, Cout).sum(0)


def contrast(x):
    """Contrast_Layer: x - avg3x3 of the one-pixel SYMMETRIC (edge repeated) pad.  Self-adjoint: this is also its backward."""
    xp = np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
    H, W = x.shape[1:3]
    s = sum(xp[:, dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3))
    return x - s / 9.0


def contrast_gate_backward(P, dP, dLC):
    return relu_gate(P, dP + contrast(dLC))


def score_backward(dscore, prob=None, dprob=None):
    """Gradient at Score = Local_Score + Global_Score with Prob = softmax(Score)[..., 0:1]: (d Local_Score [B,H,W,2], d Global_Score [B,2])."""
    d = dscore.copy()
    if dprob is not None:
        t = prob[..., 0] * (1.0 - prob[..., 0]) * dprob[..., 0]
        d[..., 0] += t
        d[..., 1] -= t
    return d, d.sum((1, 2))


# ----------------------------------------------------------------------------- the walk
def walk(acts, hw, dscore, dprob=None, dlocal_fea=None, dfea_global=None):
    """acts: pools (five [B,hw,hw,C_k]), cat1..cat5, G1, G2, Fea_Global [B,1,1,fea], Local_Fea, Prob -- float64 copies of what the
    forward left.  Returns (dpools: five arrays, dparams: {'<layer>/W' | '<layer>/b': array})."""
    f64 = lambda a: None if a is None else np.asarray(a, np.float64)
    acts = {k: ([f64(p) for p in v] if k == "pools" else f64(v)) for k, v in acts.items()}
    hw = {k: f64(v) for k, v in hw.items()}
    fea = hw["Fea_Global/W"].shape[3]
    pools = acts["pools"]
    dp = {}
    dls, dgs = score_backward(f64(dscore), acts.get("Prob"), f64(dprob))
    B = dls.shape[0]
    dp["Local_Score/b"] = dp["Global_Score/b"] = dgs.sum(0)
    # Local_Score, Global_Score (1x1)
    lf = acts["Local_Fea"]
    dp["Local_Score/W"] = (lf.reshape(-1, lf.shape[3]).T @ dls.reshape(-1, 2)).reshape(hw["Local_Score/W"].shape)
    dlf = dls @ hw["Local_Score/W"][0, 0].T
    if dlocal_fea is not None:
        dlf = dlf + f64(dlocal_fea)
    fg = acts["Fea_Global"].reshape(B, fea)
    dp["Global_Score/W"] = (fg.T @ dgs).reshape(1, 1, fea, 2)
    dfg = dgs @ hw["Global_Score/W"][0, 0].T
    if dfea_global is not None:
        dfg = dfg + f64(dfea_global).reshape(B, fea)
    dfg = dfg.reshape(B, 1, 1, fea)
    # global branch
    dp["Fea_Global/W"], dp["Fea_Global/b"] = conv_wgrad(acts["G2"], dfg, 3, 0)
    dg2 = relu_gate(acts["G2"], conv_dgrad(dfg, hw["Fea_Global/W"], 0, acts["G2"].shape[1]))
    dp["Fea_Global_2/W"], dp["Fea_Global_2/b"] = conv_wgrad(acts["G1"], dg2, 5, 0)
    dg1 = relu_gate(acts["G1"], conv_dgrad(dg2, hw["Fea_Global_2/W"], 0, acts["G1"].shape[1]))
    dp["Fea_Global_1/W"], dp["Fea_Global_1/b"] = conv_wgrad(pools[4], dg1, 5, 0)
    dpool5_global = conv_dgrad(dg1, hw["Fea_Global_1/W"], 0, pools[4].shape[1])
    # Local_Fea
    dp["Local_Fea/W"], dp["Local_Fea/b"] = conv_wgrad(acts["cat1"], dlf, 1, 0)
    dcat = conv_dgrad(dlf, hw["Local_Fea/W"], 0, lf.shape[1])
    dpools = []
    for k in range(5):
        cat = acts[f"cat{k + 1}"]
        if k < 4:
            name = f"Fea_P{k + 2}_Deconv"
            dup = relu_gate(cat[..., 2 * fea:], dcat[..., 2 * fea:])
            dnext, dp[name + "/W"], dp[name + "/b"] = deconv_backward(dup, acts[f"cat{k + 2}"], hw[name + "/W"])
        g = contrast_gate_backward(cat[..., :fea], dcat[..., :fea], dcat[..., fea:2 * fea])
        name = f"Fea_P{k + 1}"
        dp[name + "/W"], dp[name + "/b"] = conv_wgrad(pools[k], g, 3, 1)
        dpools.append(conv_dgrad(g, hw[name + "/W"], 1, pools[k].shape[1]))
        if k < 4:
            dcat = dnext
    dpools[4] = dpools[4] + dpool5_global
    return dpools, dp


# ----------------------------------------------------------------------------- the head in torch
def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def t_conv(x, W, b, pad):
    return _nhwc(F.conv2d(_nchw(x), W.permute(3, 2, 0, 1), b, padding=pad))


def t_deconv(x, W, b):
    h = x.shape[1]
    return _nhwc(F.conv_transpose2d(_nchw(x), W.permute(3, 2, 0, 1), b, stride=2, padding=1)[:, :, :2 * h, :2 * h])


def t_contrast(x):
    return _nhwc(_nchw(x) - F.avg_pool2d(F.pad(_nchw(x), (1, 1, 1, 1), mode="replicate"), 3, 1))


def gates_of(acts):
    """The ReLU masks of a forward's activations, by the names torch_forward(gates=...) reads."""
    fea = acts["Fea_Global"].shape[3]
    g = {"G1": acts["G1"] > 0, "G2": acts["G2"] > 0}
    for k in range(5):
        g[f"P{k + 1}"] = acts[f"cat{k + 1}"][..., :fea] > 0
        if k < 4:
            g[f"Up{k + 1}"] = acts[f"cat{k + 1}"][..., 2 * fea:] > 0
    return g


def torch_forward(pools, hw, gates=None):
    """The head on torch tensors `pools` (five NHWC) with variables hw ({name: tensor}): every activation `walk` reads plus Score.
    gates ({name: bool tensor}, gates_of): every ReLU is replaced by the multiplication with its fixed mask -- the smooth function whose
    derivative the backward is."""
    fea = hw["Fea_Global/W"].shape[3]
    c = lambda x, n, pad: t_conv(x, hw[n + "/W"], hw[n + "/b"], pad)
    relu = lambda z, n: torch.relu(z) if gates is None else z * gates[n].to(z.dtype)
    a = {"pools": list(pools)}
    a["G1"] = relu(c(pools[4], "Fea_Global_1", 0), "G1")
    a["G2"] = relu(c(a["G1"], "Fea_Global_2", 0), "G2")
    a["Fea_Global"] = c(a["G2"], "Fea_Global", 0)
    P = [relu(c(pools[k], f"Fea_P{k + 1}", 1), f"P{k + 1}") for k in range(5)]
    cat = torch.cat([P[4], t_contrast(P[4])], 3)
    a["cat5"] = cat
    for k in (3, 2, 1, 0):
        n = f"Fea_P{k + 2}_Deconv"
        cat = torch.cat([P[k], t_contrast(P[k]), relu(t_deconv(cat, hw[n + "/W"], hw[n + "/b"]), f"Up{k + 1}")], 3)
        a[f"cat{k + 1}"] = cat
    a["Local_Fea"] = c(a["cat1"], "Local_Fea", 0)
    a["Score"] = c(a["Local_Fea"], "Local_Score", 0) + c(a["Fea_Global"], "Global_Score", 0)
    a["Prob"] = torch.softmax(a["Score"], 3)[..., 0:1]
    assert a["Fea_Global"].shape[1:3] == (1, 1) and fea == a["Fea_Global"].shape[3]
    return a


def _vjp(fn, inputs, gout):
    ins = [t.detach().clone().requires_grad_(True) for t in inputs]
    return torch.autograd.grad(fn(*ins), ins, gout)


def torch_walk(acts, hw, dscore, dprob=None, dlocal_fea=None, dfea_global=None, dtype=torch.float32):
    """`walk` in `dtype` on the CPU from torch's own per-layer vector-Jacobian products, the gates taken from the given activations."""
    T = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    A = {k: ([T(p) for p in v] if k == "pools" else T(v)) for k, v in acts.items()}
    Wt = {k: T(v) for k, v in hw.items()}
    fea = Wt["Fea_Global/W"].shape[3]
    gate = lambda act, g: torch.where(act > 0, g, torch.zeros_like(g))
    dp = {}

    def conv_b(x, name, pad, g):
        dx, dp[name + "/W"], dp[name + "/b"] = _vjp(lambda x_, W_, b_: t_conv(x_, W_, b_, pad), (x, Wt[name + "/W"], Wt[name + "/b"]), g)
        return dx

    d = T(dscore).clone()
    if dprob is not None:
        t = A["Prob"][..., 0] * (1 - A["Prob"][..., 0]) * T(dprob)[..., 0]
        d[..., 0] += t
        d[..., 1] -= t
    B = d.shape[0]
    dgs = d.sum((1, 2)).reshape(B, 1, 1, 2)
    dlf = conv_b(A["Local_Fea"], "Local_Score", 0, d)
    if dlocal_fea is not None:
        dlf = dlf + T(dlocal_fea)
    dfg = conv_b(A["Fea_Global"], "Global_Score", 0, dgs)
    if dfea_global is not None:
        dfg = dfg + T(dfea_global).reshape(dfg.shape)
    dg2 = gate(A["G2"], conv_b(A["G2"], "Fea_Global", 0, dfg))
    dg1 = gate(A["G1"], conv_b(A["G1"], "Fea_Global_2", 0, dg2))
    dpool5_global = conv_b(A["pools"][4], "Fea_Global_1", 0, dg1)
    dcat = conv_b(A["cat1"], "Local_Fea", 0, dlf)
    dpools = []
    for k in range(5):
        cat = A[f"cat{k + 1}"]
        if k < 4:
            n = f"Fea_P{k + 2}_Deconv"
            dup = gate(cat[..., 2 * fea:], dcat[..., 2 * fea:])
            dnext, dp[n + "/W"], dp[n + "/b"] = _vjp(t_deconv, (A[f"cat{k + 2}"], Wt[n + "/W"], Wt[n + "/b"]), dup)
        g = gate(cat[..., :fea], dcat[..., :fea] + t_contrast(dcat[..., fea:2 * fea]))
        dpools.append(conv_b(A["pools"][k], f"Fea_P{k + 1}", 1, g.contiguous()))
        if k < 4:
            dcat = dnext
    dpools[4] = dpools[4] + dpool5_global
    return [p.numpy() for p in dpools], {k: v.numpy() for k, v in dp.items()}
