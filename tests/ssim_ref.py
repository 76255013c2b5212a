"""numpy restatement of the reference's image-similarity measures (utils.py: _tf_fspecial_gauss :74-89, tf_ssim :91-124, tf_ms_ssim
:126-166) and of their gradient, written from the semantics and not from the kernels: the 2-D window, direct size*size-tap sums in
the reference's order, the SAME 2x2 average pool and the all-elements reduce_prod.  Every function takes the dtype it computes in
(float32 or float64); float64 is the yardstick of the GPU tests and float32's deviation from it their unit.

Images are [B,H,W] arrays (the one channel dropped).  The gradient treats l**0 and c**0 as constants (the library's documented
departure from TensorFlow, whose 0 * c^-1 is NaN on flat windows)."""
import numpy as np

C3 = (0.03 * 1) ** 2 / 2.0


def fspecial_gauss(size, sigma, dtype=np.float64):
    """[size,size] window: offsets -size//2+1 .. size//2 (floor division), exp(-(x^2+y^2)/(2 sigma^2)) normalised by its sum."""
    c = np.arange(-size // 2 + 1, size // 2 + 1).astype(dtype)
    x, y = c[:, None], c[None, :]
    g = np.exp(-((x ** 2 + y ** 2) / dtype(2.0 * sigma ** 2))).astype(dtype)
    return (g / g.sum(dtype=dtype)).astype(dtype)


def offsets(size):
    return list(range(-size // 2 + 1, size // 2 + 1))


def conv_valid(img, win):
    """tf.nn.conv2d(img, win, VALID) (a correlation) by direct tap-by-tap sums in img's dtype; img [B,H,W]."""
    k = win.shape[0]
    oh, ow = img.shape[1] - k + 1, img.shape[2] - k + 1
    acc = np.zeros((img.shape[0], oh, ow), dtype=img.dtype)
    for a in range(k):
        for b in range(k):
            acc += win[a, b] * img[:, a:a + oh, b:b + ow]
    return acc


def conv_valid_adjoint(g, win, H, W):
    """adjoint of conv_valid with respect to the image: [B,oh,ow] -> [B,H,W]."""
    k = win.shape[0]
    oh, ow = g.shape[1], g.shape[2]
    out = np.zeros((g.shape[0], H, W), dtype=g.dtype)
    for a in range(k):
        for b in range(k):
            out[:, a:a + oh, b:b + ow] += win[a, b] * g
    return out


def _moments(x, y, win):
    mu1, mu2 = conv_valid(x, win), conv_valid(y, win)
    s1 = conv_valid(x * x, win) - mu1 * mu1
    s2 = conv_valid(y * y, win) - mu2 * mu2
    s12 = conv_valid(x * y, win) - mu1 * mu2
    return mu1, mu2, s1, s2, s12


def ssim_map(x, y, size=9, sigma=0.5, dtype=np.float64):
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    win = fspecial_gauss(size, sigma, dtype)
    _, _, s1, s2, s12 = _moments(x, y, win)
    c3 = dtype(C3)
    return ((s12 * s12 + c3) / (s1 * s2 + c3)).astype(dtype)


def tf_ssim(x, y, mean_metric=True, cs_map=False, size=9, sigma=0.5, dtype=np.float64):
    s = ssim_map(x, y, size, sigma, dtype)
    value = (np.ones_like(s), s) if cs_map else s
    if mean_metric:
        value = tuple(v.mean(dtype=dtype) for v in value) if cs_map else value.mean(dtype=dtype)
    return value


def avg_pool_same(x):
    """tf.nn.avg_pool 2x2 stride 2 SAME on [B,H,W]: ceil(n/2) outputs, a window over the edge averages the pixels that exist."""
    B, H, W = x.shape
    oh, ow = (H + 1) // 2, (W + 1) // 2
    tot = np.zeros((B, oh, ow), dtype=x.dtype)
    cnt = np.zeros((oh, ow), dtype=x.dtype)
    for di in range(2):
        for dj in range(2):
            part = x[:, di::2, dj::2]
            tot[:, :part.shape[1], :part.shape[2]] += part
            cnt[:part.shape[1], :part.shape[2]] += 1
    return (tot / cnt).astype(x.dtype)


def avg_pool_same_adjoint(g, H, W):
    oh, ow = g.shape[1], g.shape[2]
    cnt = np.zeros((oh, ow), dtype=g.dtype)
    for di in range(2):
        for dj in range(2):
            cnt[:(H - di + 1) // 2, :(W - dj + 1) // 2] += 1
    q = g / cnt
    out = np.zeros((g.shape[0], H, W), dtype=g.dtype)
    for di in range(2):
        for dj in range(2):
            n_i, n_j = (H - di + 1) // 2, (W - dj + 1) // 2
            out[:, di::2, dj::2] = q[:, :n_i, :n_j]
    return out


def level_sizes(H, W, level=5):
    out = []
    for _ in range(level):
        out.append((H, W))
        H, W = (H + 1) // 2, (W + 1) // 2
    return out


def ms_ssim_level_means(x, y, level=5, dtype=np.float64):
    """[level, B] per-sample means of the cs map at each level."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    rows = []
    for _ in range(level):
        s = ssim_map(x, y, 9, 0.5, dtype)
        rows.append(s.reshape(s.shape[0], -1).mean(axis=1, dtype=dtype))
        x, y = avg_pool_same(x), avg_pool_same(y)
    return np.stack(rows, axis=0)


def tf_ms_ssim(x, y, batch_size, mean_metric=True, level=5, dtype=np.float64):
    """ml[level-1]**1 * reduce_prod(mcs**1) with no axis: a [batch_size] vector of one repeated number (utils.py:162)."""
    assert batch_size == np.asarray(x).shape[0]
    mcs = ms_ssim_level_means(x, y, level, dtype)
    ml_last = np.ones(batch_size, dtype=dtype)
    value = (ml_last * np.prod(mcs, dtype=dtype)).astype(dtype)
    return value.mean(dtype=dtype) if mean_metric else value


# ---- gradient, closed form ---------------------------------------------------------------------------------------------------------
def ssim_grad(x, y, gmap, size=9, sigma=0.5, dtype=np.float64):
    """d/dx, d/dy of sum(gmap * s) for the upstream gradient gmap [B,oh,ow] of the map:
    ds/ds12 = 2 s12 / D, ds/ds1 = -N s2 / D^2, ds/ds2 = -N s1 / D^2; five fields through the adjoint of the VALID correlation;
    dx = A(g_mu1) + 2 x A(g_xx) + y A(g_xy), dy likewise."""
    x, y, g = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(gmap, dtype=dtype)
    win = fspecial_gauss(size, sigma, dtype)
    mu1, mu2, s1, s2, s12 = _moments(x, y, win)
    c3 = dtype(C3)
    N, D = s12 * s12 + c3, s1 * s2 + c3
    a = g * (2 * s12 / D)
    b1 = g * (-N * s2 / (D * D))
    b2 = g * (-N * s1 / (D * D))
    g_mu1 = -2 * mu1 * b1 - mu2 * a
    g_mu2 = -2 * mu2 * b2 - mu1 * a
    H, W = x.shape[1], x.shape[2]
    adj = lambda f: conv_valid_adjoint(f.astype(dtype), win, H, W)      # noqa: E731
    axy = adj(a)
    dx = adj(g_mu1) + 2 * x * adj(b1) + y * axy
    dy = adj(g_mu2) + 2 * y * adj(b2) + x * axy
    return dx.astype(dtype), dy.astype(dtype)


def ssim_mean_grad(x, y, gmeans, size=9, sigma=0.5, dtype=np.float64):
    """gradient for the upstream gradient gmeans [B] of the per-sample means"""
    x = np.asarray(x, dtype=dtype)
    oh, ow = x.shape[1] - size + 1, x.shape[2] - size + 1
    g = np.broadcast_to((np.asarray(gmeans, dtype=dtype) / dtype(oh * ow))[:, None, None], (x.shape[0], oh, ow))
    return ssim_grad(x, y, g, size, sigma, dtype)


def ms_ssim_grad(x, y, gvec, level=5, dtype=np.float64):
    """gradient of sum(gvec * tf_ms_ssim(x, y, B, mean_metric=False)): every entry is P = prod of all level*B means, so
    dP = sum(gvec) and d P / d mean[l,b] = P / mean[l,b]; each level's image gradient goes back through the pools' adjoints."""
    x, y = np.asarray(x, dtype=dtype), np.asarray(y, dtype=dtype)
    xs, ys = [x], [y]
    for _ in range(level - 1):
        xs.append(avg_pool_same(xs[-1]))
        ys.append(avg_pool_same(ys[-1]))
    means = np.stack([ssim_map(a, b, 9, 0.5, dtype).reshape(a.shape[0], -1).mean(axis=1, dtype=dtype) for a, b in zip(xs, ys)], axis=0)
    P = np.prod(means, dtype=dtype)
    dP = np.asarray(gvec, dtype=dtype).sum(dtype=dtype)
    dx = dy = None
    for lv in range(level - 1, -1, -1):
        gx, gy = ssim_mean_grad(xs[lv], ys[lv], dP * P / means[lv], 9, 0.5, dtype)
        if dx is not None:
            H, W = xs[lv].shape[1], xs[lv].shape[2]
            gx, gy = gx + avg_pool_same_adjoint(dx, H, W), gy + avg_pool_same_adjoint(dy, H, W)
        dx, dy = gx.astype(dtype), gy.astype(dtype)
    return dx, dy
