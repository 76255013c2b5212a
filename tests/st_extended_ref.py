"""numpy restatement of the spatial_transformer.py samplers that oracle/ does not cover ("ST" = the reference's
spatial_transformer.py): bicubic_interp (ST:966-1072), the symmetric-pad transformers (SimilarityTransformer ST:311-371,
AffineSymmetryTransformer ST:454-517, ProjectiveSymmetryTransformer ST:611-716) and ElasticTransformer (ST:40-224).
fp32 op by op where the kernels evaluate the same sequence; the thin-plate spline's coordinates in fp64 (the tests bound the
difference).  Unlike the kernels, this restatement materialises the padded image with np.pad(mode='symmetric') and the crop
with explicit slicing, as the reference does."""
import numpy as np

from oracle import vstab_oracle as vo

f32 = np.float32
# alpha = -0.75 (ST:967-974): rows of (1, t, t^2, t^3) coefficients
BICUBIC_COEFFS = ((1.0, 0.0, -2.25, 1.25), (0.0, -0.75, 1.5, -0.75), (0.0, 0.75, 1.5, -1.25), (0.0, 0.0, -0.75, 0.75))


def linspace(n):
    return vo.st_linspace(n)


def cubic_weights(t):
    """get_weights (ST:1038-1050): w_i = ((c_i0 + c_i1 t) + c_i2 t^2) + c_i3 t^3 in fp32."""
    t = np.asarray(t, f32)
    t2 = t * t
    t3 = t2 * t
    return [((f32(c[0]) + f32(c[1]) * t) + f32(c[2]) * t2) + f32(c[3]) * t3 for c in BICUBIC_COEFFS]


def cubic_axis(v, n):
    """ST:988-1014 along one axis: clip to [-1,1] (NaN -> -1, the kernels' rule), scale, taps [x0, x0-1, x0+1, x0+2] clamped."""
    v = np.asarray(v, f32)
    v = np.where(np.isnan(v), f32(-1), np.clip(v, f32(-1), f32(1))).astype(f32)
    v = ((v + f32(1)) / f32(2) * (f32(n) - f32(1))).astype(f32)
    v0f = np.floor(v)
    v0 = v0f.astype(np.int64)
    taps = [v0, np.maximum(v0 - 1, 0), np.minimum(v0 + 1, n - 1), np.minimum(v0 + 2, n - 1)]
    return taps, cubic_weights(v - v0f)


def bicubic_interp(im, x, y, out_size):
    """bicubic_interp (ST:966-1072).  im [B,H,W,C]; x, y flat [B*oh*ow] -> [B*oh*ow, C] fp32."""
    im = np.asarray(im, f32)
    B, H, W, C = im.shape
    npix = out_size[0] * out_size[1]
    xs, wx = cubic_axis(np.asarray(x, f32).reshape(-1), W)
    ys, wy = cubic_axis(np.asarray(y, f32).reshape(-1), H)
    n = np.repeat(np.arange(B), npix)
    rows = []
    for i in range(4):
        acc = None
        for j in range(4):
            term = wx[j][:, None] * im[n, ys[i], xs[j]]
            acc = term if acc is None else (acc + term).astype(f32)
        rows.append(acc)
    out = None
    for i in range(4):
        term = wy[i][:, None] * rows[i]
        out = term if out is None else (out + term).astype(f32)
    return out.astype(f32)


def interpolate(im, x, y, out_size, method):
    if method == 'bicubic':
        return bicubic_interp(im, x, y, out_size)
    import torch
    return vo.st_bilinear_interp(torch.from_numpy(np.asarray(im, f32)), torch.from_numpy(np.asarray(x, f32)),
                                 torch.from_numpy(np.asarray(y, f32)), out_size).numpy()


def grid(oh, ow):
    """_meshgrid (ST:755-779) as (x_t, y_t) flat [oh*ow]."""
    g = vo.st_meshgrid((oh, ow)).reshape(3, -1)
    return g[0], g[1]


def apply_matrix(th, xt, yt):
    """theta . (x_t, y_t, 1) with every product and sum rounded to fp32, (t0 x + t1 y) + t2 -- the kernels' sequence."""
    th = np.asarray(th, f32)
    xs = (th[:, 0:1] * xt + th[:, 1:2] * yt) + th[:, 2:3]
    ys = (th[:, 3:4] * xt + th[:, 4:5] * yt) + th[:, 5:6]
    if th.shape[1] == 9:
        zs = (th[:, 6:7] * xt + th[:, 7:8] * yt) + th[:, 8:9]
        xs, ys = xs / zs, ys / zs
    return xs.astype(f32), ys.astype(f32)


def transform(im, theta, out_size, method):
    """Affine/ProjectiveTransformer.transform (ST:400-452, 539-608) with either sampler; theta [B,6] or [B,8]."""
    im = np.asarray(im, f32)
    B = im.shape[0]
    th = np.asarray(theta, f32).reshape(B, -1)
    xt, yt = grid(*out_size)
    if th.shape[1] == 6:
        xs, ys = apply_matrix(th, xt, yt)
    else:
        t9 = np.concatenate([th, np.ones((B, 1), f32)], 1)
        xs, ys = apply_matrix(t9[:, :6], xt, yt)
        zs = ((t9[:, 6:7] * xt + t9[:, 7:8] * yt) + t9[:, 8:9]).astype(f32)
        zs = np.where(zs == 0, zs + f32(1e-8), zs).astype(f32)             # safe_z (ST:598)
        xs, ys = (xs / zs).astype(f32), (ys / zs).astype(f32)
    out = interpolate(im, xs.reshape(-1), ys.reshape(-1), out_size, method)
    return out.reshape(B, out_size[0], out_size[1], im.shape[3])


# ---------------------------------------------------------------------------------------------------- symmetric-pad transformers
def refl(u, n):
    """The kernels' index map of the 100-px symmetric pad: refl(p - 100, n) for a padded index p."""
    u = np.asarray(u)
    return np.where(u < 0, -u - 1, np.where(u >= n, 2 * n - 1 - u, u))


def sym_theta(kind, theta, cos=np.cos, sin=np.sin):
    """The three pre-maps in fp32: [B,6] (affine / similarity) or [B,9] (projective) matrices per sample."""
    theta = np.asarray(theta, f32)
    B = theta.shape[0]
    if kind == 'affine':                                                   # ST:502-505
        c = np.array([[.1, 0, .2], [.1, 0, .2]], f32).reshape(6)
        I = np.array([1, 0, 0, 0, 1, 0], f32)
        return ((theta.reshape(B, 6) * c) * f32(0) + I).astype(f32)
    if kind == 'projective':                                               # ST:692-699
        t9 = np.concatenate([theta.reshape(B, 8), np.ones((B, 1), f32)], 1)
        P = np.array([[0.01, 0.005, 0.01], [0.01, 0.005, 0.01], [0.01, 0.01, 1]], f32).reshape(9)
        A = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0], f32)
        return (t9 * P + A).astype(f32)
    t = (theta.reshape(B, 4) * np.array([3.14 / 6, 0.1, 0.2, 0.2], f32) + np.array([0, 1, 0, 0], f32)).astype(f32)   # ST:356-357
    a, s = t[:, 0], t[:, 1]
    ca, sa = cos(a).astype(t.dtype), sin(a).astype(t.dtype)
    flat = np.concatenate([s * ca, s * sa, t[:, 2], (-s) * sa, s * ca, t[:, 3]], 0)      # ST:358: six [B] vectors on axis 0
    return flat.reshape(B, 6)                                              # ST:360 reshape [-1,2,3]: interleaved for B > 1


def crop_or_pad(img, th, tw):
    """tf.image.resize_image_with_crop_or_pad(img [B,h,w,C], th, tw): centre crop / centre zero pad per axis."""
    B, h, w, C = img.shape
    out = np.zeros((B, th, tw, C), img.dtype)
    cy, py = max((h - th) // 2, 0), max((th - h) // 2, 0)
    cx, px = max((w - tw) // 2, 0), max((tw - w) // 2, 0)
    ly, lx = min(h, th), min(w, tw)
    out[:, py:py + ly, px:px + lx] = img[:, cy:cy + ly, cx:cx + lx]
    return out


def symmetry_transform(kind, im, theta, out_size, method, cos=np.cos, sin=np.sin):
    """SimilarityTransformer / AffineSymmetryTransformer / ProjectiveSymmetryTransformer.transform.  Returns the reference's
    shape: [B, ow, oh, C] (the affine one relabelled [B, oh, ow, C])."""
    im = np.asarray(im, f32)
    B, H, W, C = im.shape
    oh, ow = out_size
    pad = np.pad(im, ((0, 0), (100, 100), (100, 100), (0, 0)), mode='symmetric')        # ST:328, 472, 664
    M = sym_theta(kind, theta, cos, sin)
    xt, yt = grid(oh + 200, ow + 200)
    xs, ys = apply_matrix(M, xt, yt)
    out = interpolate(pad, xs.reshape(-1), ys.reshape(-1), (oh + 200, ow + 200), method).reshape(B, oh + 200, ow + 200, C)
    out = crop_or_pad(out, ow, oh)                                          # ST:343: target (out_size[1], out_size[0])
    if kind == 'affine':
        out = out.reshape(B, oh, ow, C)                                     # ST:492
    return out


def symmetry_coords64(kind, theta, out_size):
    """fp64 source coordinates of the similarity grid (cos / sin in double) for the tolerance derivation."""
    M = sym_theta(kind, theta, np.cos, np.sin).astype(np.float64)
    if kind == 'similarity':
        t = (np.asarray(theta, f32).reshape(-1, 4) * np.array([3.14 / 6, 0.1, 0.2, 0.2], f32) + np.array([0, 1, 0, 0], f32)).astype(np.float64)
        a, s = t[:, 0], t[:, 1]
        M = np.concatenate([s * np.cos(a), s * np.sin(a), t[:, 2], -s * np.sin(a), s * np.cos(a), t[:, 3]], 0).reshape(-1, 6)
    xt, yt = grid(out_size[0] + 200, out_size[1] + 200)
    xt, yt = xt.astype(np.float64), yt.astype(np.float64)
    return M[:, 0:1] * xt + M[:, 1:2] * yt + M[:, 2:3], M[:, 3:4] * xt + M[:, 4:5] * yt + M[:, 5:6]


# ---------------------------------------------------------------------------------------------------- thin-plate spline
def tps_source_points(g):
    """get_meshgrid(g, g) (ST:176-184): [2, K], x fastest, fp32 linspace."""
    xp, yp = np.meshgrid(linspace(g), linspace(g))
    return np.stack([xp.reshape(-1), yp.reshape(-1)]).astype(f32)


def tps_U(r2):
    """U_func (ST:162-172): r^2 log r^2, 0 where r^2 = 0."""
    r2 = np.asarray(r2, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(r2 == 0, 0.0, r2 * np.log(np.where(r2 == 0, 1.0, r2)))


def tps_L(g):
    """_initialize_tps's L (ST:204-211), (K+3) x (K+3), in fp64 from the fp32 control points; row 2 is [0, 0, 1, ..., 1]."""
    p = tps_source_points(g).astype(np.float64)
    K = g * g
    d = p[:, :, None] - p[:, None, :]
    tL = tps_U((d ** 2).sum(0)).T
    top = np.concatenate([np.zeros((2, 3)), p], 1)
    mid = np.concatenate([np.zeros((1, 2)), np.ones((1, K + 1))], 1)
    bot = np.concatenate([p.T, np.ones((K, 1)), tL], 1)
    return np.concatenate([top, mid, bot], 0)


def tps_linv_t(g):
    """transpose(inv(L)[:, 3:]) [K, K+3] in fp64 (ST:212, 223)."""
    return np.linalg.inv(tps_L(g))[:, 3:].T.copy()


def tps_coords(theta, g, out_size, linv_t):
    """ElasticTransformer._transform (ST:140-158) in fp64 given the table linv_t [K, K+3]: coeff = (source + theta) . linv_t,
    then coeff . [x_t, y_t, 1, U_1..U_K] on the (oh, ow) grid.  Also returns the per-pixel sums of |terms| (for the bounds)."""
    K = g * g
    B = np.asarray(theta).reshape(-1, 2 * K).shape[0]
    P = (tps_source_points(g)[None] + np.asarray(theta, f32).reshape(B, 2, K)).astype(f32).astype(np.float64)   # ST:108, in fp32
    Lt = np.asarray(linv_t, np.float64)
    coeff = P @ Lt                                                          # [B, 2, K+3]
    coeff_abs = np.abs(P) @ np.abs(Lt)
    xt, yt = grid(*out_size)
    src = tps_source_points(g).astype(np.float64)
    xt64, yt64 = xt.astype(np.float64), yt.astype(np.float64)
    U = tps_U((xt64[None] - src[0][:, None]) ** 2 + (yt64[None] - src[1][:, None]) ** 2)        # [K, N]
    r2 = (xt64[None] - src[0][:, None]) ** 2 + (yt64[None] - src[1][:, None]) ** 2
    R = np.concatenate([xt64[None], yt64[None], np.ones((1, xt.size)), U], 0)                  # [K+3, N]
    T = coeff @ R                                                           # [B, 2, N]
    # |terms| with |U| + r^2 for the U rows: an fp32 U = r^2 ln r^2 is off by a few ulp of |U| plus a few ulp of r^2 (ln near 0)
    Tabs = np.abs(coeff) @ np.concatenate([np.abs(R[:3]), np.abs(U) + r2], 0)
    Tcoef = coeff_abs @ np.abs(R)
    return T[:, 0], T[:, 1], Tabs, Tcoef
