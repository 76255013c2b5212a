"""Float64 numpy reference of the VGG16 trunk and its backward, NHWC tensors and HWIO filters as vgg16.py
holds them: conv 3x3 SAME + bias, ReLU, max-pool 2x2 stride 2 SAME.  Two rules fix the backward where calculus does not:
  tie rule   a pool window's gradient goes to its first maximum in the order (0,0), (0,1), (1,0), (1,1) among the taps inside the
             image;
  zero rule  a gradient passes a ReLU only where its output is > 0, so a window whose maximum is 0 passes nothing.
`torch_backward` is the same network under torch.autograd (F.conv2d / relu / max_pool2d(2, 2, ceil_mode=True)) in a chosen dtype:
the independent check of this file in float64, and the float32 yardstick of the GPU tests."""
import numpy as np

LAYERS = (("conv1_1", 3, 64, False), ("conv1_2", 64, 64, True), ("conv2_1", 64, 128, False), ("conv2_2", 128, 128, True),
          ("conv3_1", 128, 256, False), ("conv3_2", 256, 256, False), ("conv3_3", 256, 256, True), ("conv4_1", 256, 512, False),
          ("conv4_2", 512, 512, False), ("conv4_3", 512, 512, True), ("conv5_1", 512, 512, False), ("conv5_2", 512, 512, False),
          ("conv5_3", 512, 512, True))
OUTPUTS = tuple(n for name, _, _, pool in LAYERS for n in ((name, "pool" + name[4]) if pool else (name,)))


def _cols(x):
    """[B,H,W,C] -> [B*H*W, 9*C], taps in (ky, kx, c) order, zero padding 1."""
    B, H, W, C = x.shape
    xp = np.zeros((B, H + 2, W + 2, C), dtype=x.dtype)
    xp[:, 1:-1, 1:-1] = x
    return np.concatenate([xp[:, ky:ky + H, kx:kx + W] for ky in range(3) for kx in range(3)], axis=3).reshape(B * H * W, 9 * C)


def conv_forward(x, Wf, b):
    B, H, W, _ = x.shape
    return (_cols(x) @ Wf.reshape(-1, Wf.shape[3]) + b).reshape(B, H, W, Wf.shape[3])


def conv_backward(x, Wf, gz, need_dx=True):
    """Gradients of conv_forward at its output gradient gz: (dx or None, dW, db)."""
    B, H, W, ci = x.shape
    co = Wf.shape[3]
    g2 = gz.reshape(B * H * W, co)
    dW = (_cols(x).T @ g2).reshape(3, 3, ci, co)
    db = g2.sum(axis=0)
    if not need_dx:
        return None, dW, db
    dcols = (g2 @ Wf.reshape(-1, co).T).reshape(B, H, W, 9, ci)
    dxp = np.zeros((B, H + 2, W + 2, ci), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            dxp[:, ky:ky + H, kx:kx + W] += dcols[:, :, :, ky * 3 + kx]
    return dxp[:, 1:-1, 1:-1], dW, db


def _windows(y):
    """[B,H,W,C] -> ([B,oh,ow,4,C] taps in the tie rule's order, -inf beyond the image), oh, ow"""
    B, H, W, C = y.shape
    oh, ow = (H + 1) // 2, (W + 1) // 2
    yp = np.full((B, 2 * oh, 2 * ow, C), -np.inf, dtype=y.dtype)
    yp[:, :H, :W] = y
    return yp.reshape(B, oh, 2, ow, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, oh, ow, 4, C), oh, ow


def pool_forward(y):
    return _windows(y)[0].max(axis=3)


def pool_relu_backward(y, dpool):
    """The gradient at y (a ReLU's output) of max_pool(2, 2, SAME)(y), gated by y > 0: the tie rule and the zero rule."""
    B, H, W, C = y.shape
    win, oh, ow = _windows(y)
    first = win.argmax(axis=3)                                   # numpy's argmax: the first maximum
    d = (np.arange(4).reshape(1, 1, 1, 4, 1) == first[:, :, :, None, :]) * dpool[:, :, :, None, :]
    d = d.reshape(B, oh, ow, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * oh, 2 * ow, C)[:, :H, :W]
    return d * (y > 0)


def forward(x, params):
    """x [B,H,W,3], params {layer: [W (3,3,ci,co), b (co,)]} -> the 18 outputs in OUTPUTS order (float64)."""
    cur = np.asarray(x, dtype=np.float64)
    outs = []
    for name, _, _, pool in LAYERS:
        cur = np.maximum(conv_forward(cur, np.asarray(params[name][0], np.float64), np.asarray(params[name][1], np.float64)), 0.0)
        outs.append(cur)
        if pool:
            cur = pool_forward(cur)
            outs.append(cur)
    return outs


def backward(x, params, grads, outs=None):
    """grads {name in OUTPUTS: gradient} at any subset of the outputs -> (dinput, {layer: (dW, db)}) for all 13 layers (zeros above
    the deepest gradient)."""
    x = np.asarray(x, dtype=np.float64)
    outs = forward(x, params) if outs is None else outs
    g_at = {n: np.asarray(g, dtype=np.float64) for n, g in grads.items()}
    assert g_at and all(n in OUTPUTS for n in g_at)
    dparams = {name: (np.zeros((3, 3, ci, co)), np.zeros(co)) for name, ci, co, _ in LAYERS}
    run = None
    for name, ci, co, pool in reversed(LAYERS):
        oc = OUTPUTS.index(name)
        y = outs[oc]
        g = None
        if pool:
            gp = g_at.get(OUTPUTS[oc + 1])
            if run is not None:
                gp = run if gp is None else run + gp
            if gp is not None:
                g = pool_relu_backward(y, gp)
            if name in g_at:
                g = g_at[name] * (y > 0) + (0.0 if g is None else g)
        else:
            g = g_at.get(name)
            if run is not None:
                g = run if g is None else run + g
            if g is not None:
                g = g * (y > 0)
        if g is None:
            continue
        xin = x if oc == 0 else outs[oc - 1]
        run, dW, db = conv_backward(xin, np.asarray(params[name][0], np.float64), g)
        dparams[name] = (dW, db)
    return run, dparams


def torch_backward(x, params, grads, dtype):
    """The same quantities from torch.autograd on the CPU in `dtype`: (dinput, {layer: (dW, db)}, outs) as float64 numpy."""
    import torch
    import torch.nn.functional as F

    xt = torch.tensor(np.asarray(x), dtype=dtype).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    P = {name: (torch.tensor(np.asarray(params[name][0]), dtype=dtype).permute(3, 2, 0, 1).contiguous().requires_grad_(True),
                torch.tensor(np.asarray(params[name][1]), dtype=dtype).requires_grad_(True)) for name, _, _, _ in LAYERS}
    cur, outs = xt, {}
    for name, _, _, pool in LAYERS:
        cur = F.relu(F.conv2d(cur, P[name][0], P[name][1], padding=1))
        outs[name] = cur
        if pool:
            cur = F.max_pool2d(cur, 2, 2, ceil_mode=True)
            outs["pool" + name[4]] = cur
    loss = sum((outs[n] * torch.tensor(np.asarray(g), dtype=dtype).permute(0, 3, 1, 2)).sum() for n, g in grads.items())
    loss.backward()
    z = lambda t, like: (torch.zeros_like(like) if t is None else t).detach().double().numpy()
    dparams = {name: (z(W.grad, W).transpose(2, 3, 1, 0), z(b.grad, b)) for name, (W, b) in P.items()}
    return (xt.grad.double().numpy().transpose(0, 2, 3, 1), dparams,
            [outs[n].detach().double().numpy().transpose(0, 2, 3, 1) for n in OUTPUTS])


def tie_plane():
    """The hand-made 3x3 plane of the tie / zero rules, one channel: y, dpool (2x2) and the dy the rules give.
       y = 5 5 2     window (0,0): a positive four-way tie      -> its gradient lands on (0,0)
           5 5 2     window (0,1): clipped right column, 2 = 2  -> on (0,2)
           0 0 3     window (1,0): all zero                     -> nowhere;  window (1,1): the single tap (2,2)"""
    y = np.array([[5., 5., 2.], [5., 5., 2.], [0., 0., 3.]])
    dpool = np.array([[1., 10.], [100., 1000.]])
    dy = np.array([[1., 0., 10.], [0., 0., 0.], [0., 0., 1000.]])
    return y, dpool, dy
