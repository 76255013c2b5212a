"""Plain references for the elementwise and reduction block of the training step (csrc/train_ops.hip behind csrc/train_api.cpp):
BatchNormLayer(act = lrelu 0.1, is_train = True) forward and backward, the bare leaky-ReLU gate, the adjoints of the decoder's two
resamplers, and axpby.  tests/test_train_kernels_ref_cpu.py anchors them on the CPU (autograd, finite differences, adjoint identities,
planted mistakes); tests/test_gpu_bn_train_kernels.py and tests/test_gpu_resampler_adjoints.py compare the kernels with them.

Every function exists twice.  dtype = np.float64 is the REFERENCE: two-pass statistics, the derivative of the forward from the true z.
dtype = np.float32 is the YARDSTICK: the kernel's own statement sequence with one IEEE rounding per operation (the library is built
with -ffp-contract=off), its sums added in the kernel's order (`kernel_order_sum`).  An error is expressed in UNITS of 2^-24 times the
sum of the absolute values of the terms added (train_kernels_ref's unit), per output:

    save_mean     mean_r |z|
    save_rstd     rstd                                         (a relative error)
    moving_*      |moving * decay| + |batch * (1 - decay)|
    y             A = (|z| + |mean|) rstd + |beta|             (u = (z - mean) rstd + beta; y = max(u, 0.1 u))
    dbeta         sum_r |g| (+ |prior| when accumulating)      (g = dy * (y > 0 ? 1 : 0.1))
    dz            rstd (|g| + mean_r |g| + X mean_r (|g| X))   with X = A + |beta|

X is what was added to form the xhat the backward works with: the kernel keeps no pre-activation and recovers xhat = y / slope - beta
from the float32 y, so xhat carries the rounding of u (relative to A) and of the subtraction (relative to |u| + |beta| <= X); X >= |xhat|
bounds both the factor and the summand of the xhat * sum(g xhat) term.  Where beta is large next to xhat the recovery loses the
digits that beta occupies, and the unit says so.  The gate (y > 0) is data: the fp64 backward takes it from the y it is handed (a sign
cannot be "nearly right") and everything else from the true z.

BN_FP32_UNITS are the largest errors of the yardstick over BN_CASES, measured by tests/test_train_kernels_ref_cpu.py (which fails
when they no longer hold); the GPU may use GPU_FACTOR = 4 times as much: the project's standing factor for a device square root and
division that need not be correctly rounded and for another summation order.  The same holds for BILINEAR_FP32_UNITS."""
import numpy as np
import torch

from oracle import vstab_oracle as vo

EPS32 = 2.0 ** -24
GPU_FACTOR = 4.0
F32, F64 = np.float32, np.float64


# ----------------------------------------------------------------------------- the two-stage column reduction
def chunk_plan(rows, C):
    """(chunks, rows per chunk) of reduce_chunks (csrc/vstab_internal.h): clamp(rows / 128, 1, max(8, 768 / column blocks))."""
    colblocks = (C + 63) // 64 if C >= 64 else 1
    n = min(max(768 // colblocks, 8), rows // 128)
    chunks = max(n, 1)
    return chunks, -(-rows // chunks)


def kernel_order_sum(v, dtype):
    """Column sums of v [rows, C] in `dtype`, added as bn_moments_kernel / bn_bwd_colsum_kernel and their final stages add them: within
    chunk k wave w adds rows k rpc + w, + 4, + 8, ... in turn; the four waves are added (0 + 1) + (2 + 3); wave w of the final stage adds
    chunks w, w + 16, ... in turn; the sixteen are added in order.  (Padding with zeros changes no sum.)"""
    v = np.asarray(v).astype(dtype)
    rows, C = v.shape
    chunks, rpc = chunk_plan(rows, C)
    steps = -(-rpc // 4)
    i = np.arange(steps * 4)
    idx = np.arange(chunks)[:, None] * rpc + i[None, :]
    valid = (i[None, :] < rpc) & (idx < rows)
    P = np.where(valid[..., None], v[np.minimum(idx, rows - 1)], dtype(0)).reshape(chunks, steps, 4, C)
    acc = np.zeros((chunks, 4, C), dtype)
    for j in range(steps):
        acc = acc + P[:, j]
    part = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])
    steps2 = -(-chunks // 16)
    Q = np.zeros((steps2 * 16, C), dtype)
    Q[:chunks] = part
    Q = Q.reshape(steps2, 16, C)
    acc2 = np.zeros((16, C), dtype)
    for j in range(steps2):
        acc2 = acc2 + Q[j]
    s = np.zeros(C, dtype)
    for w in range(16):
        s = s + acc2[w]
    return s


def addition_chain(rows, C):
    """The longest chain of additions a row's value passes through in the two stages: ceil(rpc / 4) rows of one wave within a chunk,
    2 for the four-wave add (0 + 1) + (2 + 3), ceil(chunks / 16) chunks of one final-stage wave, 16 for the sixteen-wave add."""
    chunks, rpc = chunk_plan(rows, C)
    return -(-rpc // 4) + 2 + -(-chunks // 16) + 16


def rstd_cancellation_bound(z, eps):
    """Bound on |rstd_kernel - rstd| / rstd per channel of z [rows, C] against the fp64 two-pass variance:

        (addition_chain + 3) 2^-53 E[z^2] / (var + eps) + 2^-24

    The kernel forms var = q / R - m^2 from two double sums.  z^2 of a float32 is exact in double, so q carries only its additions'
    error: every term is positive, so at most chain 2^-53 relative to q, that is chain 2^-53 E[z^2] in q / R.  The + 3 are the
    multiplication by 1 / R, the product m m and the subtraction, each one rounding of a number no larger than E[z^2].  s carries
    chain 2^-53 relative to sum |z|, and m^2 twice that, at most 2 chain 2^-53 E[z^2] (Cauchy-Schwarz).  rstd = (var + eps)^-1/2 moves
    by HALF of delta var / (var + eps), so with every contribution pulling the same way |delta rstd| / rstd <= (1.5 chain + 1.5)
    2^-53 E[z^2] / (var + eps).  The bound asserted drops that half and in exchange counts the chain once: it is the first-order worst
    case of q's share alone and two thirds of the worst case of all three, which independent roundings do not come near (they add
    like sqrt(chain)).  The float32 cast of the result adds 2^-24; the double square root and division vanish next to it."""
    z = np.asarray(z, F64)
    rows, C = z.shape
    var = ((z - z.mean(axis=0)) ** 2).mean(axis=0)
    return (addition_chain(rows, C) + 3) * 2.0 ** -53 * (z * z).mean(axis=0) / (var + float(F32(eps))) + EPS32


# ----------------------------------------------------------------------------- BatchNorm + lrelu, training mode
def bn_train_forward_ref(z, beta, eps, decay, moving_mean, moving_var, dtype=np.float64):
    """z [rows, C], beta [C] -> dict(y, mean, rstd, var, moving_mean, moving_var) in `dtype`; moving_* may be None.
    np.float64: mean and POPULATION variance in two passes, u = (z - mean) rstd + beta with rstd = 1 / sqrt(var + eps) (eps INSIDE the
    root, tf.nn.batch_normalization), y = max(u, 0.1 u), moving = moving decay + batch (1 - decay).  eps and decay are the float32
    numbers the kernel receives.
    np.float32: the kernel's sequence.  bn_moments_final_kernel: s and q = sum z^2 in double in the kernel's order, m = s / R,
    var = max(q / R - m m, 0), mean = (float)m, rstd = (float)(1 / sqrt(var + (double)eps)), moving_mean = moving_mean * decay +
    (float)m * (1.f - decay), moving_var likewise from (float)var; bn_lrelu_apply_kernel: u = (z - mean) * rstd + beta and
    y = fmaxf(u, 0.1f * u), one float32 rounding each."""
    z = np.asarray(z)
    rows = z.shape[0]
    eps64, decay32 = F64(F32(eps)), F32(decay)
    z64 = z.astype(F64)
    out = {}
    if dtype == np.float64:
        mean = z64.mean(axis=0)
        var = ((z64 - mean) ** 2).mean(axis=0)
        rstd = 1.0 / np.sqrt(var + eps64)
        u = (z64 - mean) * rstd + np.asarray(beta, F64)
        y = np.maximum(u, 0.1 * u)
        d = F64(decay32)
        mm = None if moving_mean is None else np.asarray(moving_mean, F64) * d + mean * (1.0 - d)
        mv = None if moving_var is None else np.asarray(moving_var, F64) * d + var * (1.0 - d)
    else:
        inv_rows = 1.0 / F64(rows)
        s, q = kernel_order_sum(z64, F64), kernel_order_sum(z64 * z64, F64)
        m = s * inv_rows
        var = np.maximum(q * inv_rows - m * m, 0.0)
        mean, rstd = m.astype(F32), (1.0 / np.sqrt(var + eps64)).astype(F32)
        one = F32(1.0)
        mm = None if moving_mean is None else np.asarray(moving_mean, F32) * decay32 + mean * (one - decay32)
        mv = None if moving_var is None else np.asarray(moving_var, F32) * decay32 + var.astype(F32) * (one - decay32)
        u = (z.astype(F32) - mean) * rstd + np.asarray(beta, F32)
        y = np.maximum(u, F32(0.1) * u)
    out.update(y=y, mean=mean, rstd=rstd, var=var, moving_mean=mm, moving_var=mv)
    return out


def bn_train_backward_ref(y, dy, beta, rstd, dtype=np.float64, z=None, eps=None):
    """(dz [rows, C], dbeta [C]) in `dtype`.
    np.float64 needs the true z and eps: xhat = (z - mean) rstd from the two-pass statistics of z (the `rstd` argument is not used),
    g = dy * (y > 0 ? 1 : 0.1) with the gate of the y handed in, dbeta = sum g, dz = rstd (g - mean g - xhat mean(g xhat)): the
    derivative of bn_train_forward_ref.
    np.float32 restates the kernels: g = y > 0 ? dy : 0.1f * dy; xhat = (y > 0 ? y : y / 0.1f) - beta; the sums of g and of g * xhat in
    the kernel's order; dz = rstd * (g - sum_g * (1.f / R) - xhat * (sum_gx * (1.f / R))).  At y == 0 (either sign of zero) the
    kernel's rule is slope 0.1 and xhat = -beta."""
    y = np.asarray(y)
    rows = y.shape[0]
    pos = y > 0
    if dtype == np.float64:
        z64 = np.asarray(z, F64)
        mean = z64.mean(axis=0)
        var = ((z64 - mean) ** 2).mean(axis=0)
        r = 1.0 / np.sqrt(var + F64(F32(eps)))
        xhat = (z64 - mean) * r
        g = np.asarray(dy, F64) * np.where(pos, 1.0, 0.1)
        return r * (g - g.mean(axis=0) - xhat * (g * xhat).mean(axis=0)), g.sum(axis=0)
    y, dy, beta, rstd = (np.asarray(a, F32) for a in (y, dy, beta, rstd))
    tenth = F32(0.1)
    g = np.where(pos, dy, tenth * dy)
    xhat = np.where(pos, y, y / tenth) - beta
    sg, sgx = kernel_order_sum(g, F32), kernel_order_sum(g * xhat, F32)
    inv_rows = F32(1.0) / F32(rows)
    return rstd * (g - sg * inv_rows - xhat * (sgx * inv_rows)), sg


def lrelu_backward_ref(y, dy):
    """lrelu_bwd_kernel in float32: dy where y > 0, else one rounding of dy * 0.1f."""
    y, dy = np.asarray(y, F32), np.asarray(dy, F32)
    return np.where(y > 0, dy, dy * F32(0.1))


def _worst(got, want, unit):
    got = np.asarray(got, F64)
    e = np.abs(got - want) / unit
    return float(np.where(np.isfinite(got), e, np.inf).max())


def bn_forward_errors(got, z, beta, eps, decay, moving_mean, moving_var):
    """Largest error, in units (module docstring), of each entry of `got` (as bn_train_forward_ref returns them; a None entry is
    skipped) against the fp64 reference.  Anything not finite counts as infinitely wrong."""
    want = bn_train_forward_ref(z, beta, eps, decay, moving_mean, moving_var, F64)
    z64, d = np.asarray(z, F64), F64(F32(decay))
    A = (np.abs(z64) + np.abs(want["mean"])) * want["rstd"] + np.abs(np.asarray(beta, F64))
    units = {"y": A, "mean": np.abs(z64).mean(axis=0), "rstd": want["rstd"]}
    if moving_mean is not None:
        units["moving_mean"] = np.abs(np.asarray(moving_mean, F64) * d) + np.abs(want["mean"] * (1.0 - d))
    if moving_var is not None:
        units["moving_var"] = np.abs(np.asarray(moving_var, F64) * d) + np.abs(want["var"] * (1.0 - d))
    return {k: _worst(got[k], want[k], EPS32 * u) for k, u in units.items() if got.get(k) is not None}


def bn_backward_errors(got_dz, got_dbeta, y, z, dy, beta, eps, prior=None):
    """Largest error in units of dz and (unless None) dbeta against the fp64 backward from the true z, gate taken from y; `prior` is
    what dbeta held before an accumulating call."""
    want_dz, want_db = bn_train_backward_ref(y, dy, beta, None, F64, z=z, eps=eps)
    fwd = bn_train_forward_ref(z, beta, eps, 0.0, None, None, F64)
    z64, b = np.asarray(z, F64), np.abs(np.asarray(beta, F64))
    X = (np.abs(z64) + np.abs(fwd["mean"])) * fwd["rstd"] + 2.0 * b
    ag = np.abs(np.asarray(dy, F64)) * np.where(np.asarray(y) > 0, 1.0, 0.1)
    unit_dz = fwd["rstd"] * (ag + ag.mean(axis=0) + X * (ag * X).mean(axis=0))
    out = {"dz": _worst(got_dz, want_dz, EPS32 * unit_dz)}
    if got_dbeta is not None:
        p = 0.0 if prior is None else np.asarray(prior, F64)
        out["dbeta"] = _worst(got_dbeta, want_db + p, EPS32 * (ag.sum(axis=0) + np.abs(p)))
    return out


# (rows, cs, c_off, C): each a point where reduce_chunks, the wave tails or the column blocks change behaviour
BN_CASES = [
    (1, 4, 0, 4),                # variance 0: rstd = 1 / sqrt(eps), y = lrelu(beta)
    (13, 8, 4, 4), (16, 8, 4, 4), (17, 8, 4, 4), (127, 8, 4, 4),      # around the in-flight loop's bound r + 12 < r1, one chunk
    (255, 12, 4, 8), (256, 12, 4, 8), (257, 12, 4, 8),                # one chunk turning into two
    (1000, 72, 4, 68),           # the second column block holds four channels
    (2049, 200, 0, 200),         # four column blocks, the last ragged; 16 chunks
    (2177, 64, 0, 64),           # 17 chunks: the final stages' k + 16 < chunks loop runs once
    (12801, 640, 0, 640),        # ten column blocks; 76 chunks: final-stage loop and tail
    (98311, 8, 4, 4),            # the workload's 768 chunks of 129 rows: chunk 762 holds 13 rows, 763..767 none
]
BN_EXACT_CASES = [(256, 12, 4, 8), (4096, 72, 4, 68)]


def bn_case(rows, cs, c_off, C):
    """Random data of one bounded case, both lrelu branches taken: z [rows, C] (mean 0.5, deviation 2), beta, moving_mean, moving_var,
    dy [rows, C] as float32 arrays, and (eps, decay): eps alternates between 1e-5 and 1e-3, decay between 0.9 and 0.99."""
    rng = np.random.default_rng(5000 + rows + C)
    z = (rng.standard_normal((rows, C)) * 2 + 0.5).astype(F32)
    beta = (rng.standard_normal(C) * 0.3).astype(F32)
    mm, mv = rng.standard_normal(C).astype(F32), (rng.random(C) + 0.5).astype(F32)
    dy = rng.standard_normal((rows, C)).astype(F32)
    k = [c[0] for c in BN_CASES].index(rows) if (rows, cs, c_off, C) in BN_CASES else 0
    return z, beta, mm, mv, dy, (1e-5, 1e-3)[k % 2], (0.9, 0.99)[(k // 2) % 2]


def bn_exact_integer_case(rows, C):
    """Integer z in [-4, 4] and a power-of-two row count: both double sums are exact in any order and 1 / rows is exact, so m and var
    are the exact rationals, the same doubles in one pass and in two, and mean, rstd and moving_mean of the kernel must equal the fp64
    reference cast to float32 (moving_mean: integer multiples of 4 as the prior and decay = 0.75 keep the float32 update exact)."""
    assert rows & (rows - 1) == 0
    rng = np.random.default_rng(6000 + rows + C)
    z = rng.integers(-4, 5, (rows, C)).astype(F32)
    beta = rng.integers(-2, 3, C).astype(F32)
    mm, mv = (4 * rng.integers(-8, 9, C)).astype(F32), (4 * rng.integers(1, 9, C)).astype(F32)
    return z, beta, mm, mv, 1e-5, 0.75


def bn_exact_pm_case(rows, C):
    """Half of each channel +a and half -a (a = 2^-2 .. 2^2 by channel, the places shuffled) and eps = 0: mean 0, var = a^2 and
    rstd = 1 / a exactly, xhat = +-1.  beta is an integer >= 3, so every u = xhat + beta > 0 and y = u exactly; dy holds integers in
    [-3, 3].  Then g = dy, xhat = y - beta, both backward sums are integers, and with a power-of-two row count dz and dbeta are exact.
    Returns z, beta, moving_mean, moving_var, dy, eps, decay and asserts that the sums stay below 2^24."""
    assert rows & (rows - 1) == 0 and rows >= 2
    rng = np.random.default_rng(7000 + rows + C)
    a = (2.0 ** (np.arange(C) % 5 - 2)).astype(F32)
    sign = np.concatenate([np.ones((rows // 2, C)), -np.ones((rows // 2, C))])
    sign = rng.permuted(sign, axis=0)
    z = (sign * a).astype(F32)
    beta = rng.integers(3, 7, C).astype(F32)
    mm, mv = (4 * rng.integers(-8, 9, C)).astype(F32), (4 * rng.integers(1, 9, C)).astype(F32)
    dy = rng.integers(-3, 4, (rows, C)).astype(F32)
    assert float(np.abs(dy).sum(axis=0).max()) < 2 ** 24          # bounds sum |g| and sum |g xhat|, |xhat| = 1
    return z, beta, mm, mv, dy, 0.0, 0.75


def bn_cancellation_case(kind, rows, C):
    """z [rows, C] float32 for the cancellation test.  "near_4096": mean about 4096 and a spread of a few float32 ulps there
    (ulp = 2^-11, deviation 1 .. 4 ulps by channel), so that var = 2.4e-7 .. 3.8e-6 is comparable to eps = 1e-5 while E[z^2] = 1.7e7:
    q / R - m^2 cancels 13 decimal digits.  "plain": mean 0.5, deviation 2."""
    rng = np.random.default_rng(8000 + rows + C + len(kind))
    if kind == "near_4096":
        k = np.rint(rng.standard_normal((rows, C)) * (1 + np.arange(C) % 4))
        return (4096.0 + k * 2.0 ** -11).astype(F32)
    return (rng.standard_normal((rows, C)) * 2 + 0.5).astype(F32)


# Largest error of the float32 yardstick over BN_CASES, in units; measured (tests/test_train_kernels_ref_cpu.py::
# test_bn_fp32_yardstick_sets_the_bounds) 2.8337, 0.3120, 0.9956, 1.5943, 1.6866, 2.4989, 1.1530
BN_FP32_UNITS = {"y": 2.84, "mean": 0.32, "rstd": 1.00, "moving_mean": 1.60, "moving_var": 1.69, "dz": 2.50, "dbeta": 1.16}
BN_BOUND = {k: GPU_FACTOR * u for k, u in BN_FP32_UNITS.items()}


# ----------------------------------------------------------------------------- resampler adjoints
def legacy_axis_matrix(n_in, n_out, dtype=np.float64):
    """A [n_out, n_in] of one axis of vo.resize_bilinear_legacy, out = A in: row o holds 1 - t at lo and t at hi (their sum where
    lo == hi), from the oracle's index map.  In float32 these are the kernel's own weights (lo == i ? 1.f - t : 0.f) + (hi == i ? t : 0.f)."""
    lo, hi, t = vo._legacy_axis(n_in, n_out)
    lo = np.minimum(lo, n_in - 1)
    A = np.zeros((n_out, n_in), dtype)
    o = np.arange(n_out)
    t = t.astype(dtype)
    np.add.at(A, (o, lo), dtype(1.0) - t)
    np.add.at(A, (o, hi), t)
    return A


def resize_bilinear_forward_ref(x, oh, ow):
    """fp64 forward as the explicit matrices: out[b,o,p,c] = sum Ay[o,i] Ax[p,j] x[b,i,j,c]."""
    x = np.asarray(x, F64)
    return np.einsum("oi,pj,bijc->bopc", legacy_axis_matrix(x.shape[1], oh), legacy_axis_matrix(x.shape[2], ow), x)


def resize_bilinear_backward_ref(dout, h, w, gain=1.0, prior=None, dtype=np.float64):
    """din [B,h,w,C] = (prior +) gain * A^T dout for dout [B,oh,ow,C].  np.float64: the transposed matrices.  np.float32:
    resize_bilinear_bwd_kernel's sequence, s += wy * wx * g over oy, then ox, ascending (a zero weight adds an exact zero, as skipping
    it does), then prior + gain * s."""
    dout = np.asarray(dout)
    B, oh, ow, C = dout.shape
    Ay, Ax = legacy_axis_matrix(h, oh, dtype), legacy_axis_matrix(w, ow, dtype)
    if dtype == np.float64:
        s = np.einsum("oi,pj,bopc->bijc", Ay, Ax, dout.astype(F64))
        g = F64(F32(gain))
    else:
        d32 = dout.astype(F32)
        s = np.zeros((B, h, w, C), F32)
        for oy in range(oh):
            for ox in range(ow):
                wgt = Ay[oy][:, None] * Ax[ox][None, :]
                s = s + wgt[None, :, :, None] * d32[:, oy, ox][:, None, None, :]
        g = F32(gain)
    return g * s if prior is None else np.asarray(prior, dtype) + g * s


def resize_bilinear_backward_units(dout, h, w, gain=1.0, prior=None):
    """The unit of each element of the adjoint: 2^-24 (|prior| + |gain| A^T |dout|)."""
    u = np.abs(resize_bilinear_backward_ref(np.abs(np.asarray(dout, F64)), h, w, abs(gain)))
    return EPS32 * (u if prior is None else u + np.abs(np.asarray(prior, F64)))


def pad_nearest_index(n_src, n_out):
    """Source index per output index of pad(1) + nearest(align_corners) along one axis, -1 where the zero ring is read."""
    i = vo.nearest_align_corners_index(n_src + 2, n_out) - 1
    return np.where((i >= 0) & (i < n_src), i, -1)


def pad_nearest_upsample_ref(src, H, W):
    """out[b,y,x] = src[b, iy[y], ix[x]], zero where either index falls on the ring: an indexed copy, in src's dtype."""
    src = np.asarray(src)
    iy, ix = pad_nearest_index(src.shape[1], H), pad_nearest_index(src.shape[2], W)
    out = src[:, np.maximum(iy, 0)][:, :, np.maximum(ix, 0)].copy()
    out[:, iy < 0] = 0
    out[:, :, ix < 0] = 0
    return out


def pad_nearest_upsample_backward_ref(dout, h2, w2):
    """fp64 adjoint by a scatter loop over the forward's index map: dsrc[b, iy[y], ix[x]] += dout[b, y, x]."""
    dout = np.asarray(dout, F64)
    B, H, W, C = dout.shape
    iy, ix = pad_nearest_index(h2, H), pad_nearest_index(w2, W)
    dsrc = np.zeros((B, h2, w2, C))
    for y in range(H):
        for x in range(W):
            if iy[y] >= 0 and ix[x] >= 0:
                dsrc[:, iy[y], ix[x]] += dout[:, y, x]
    return dsrc


PAD_NEAREST_CASES = [            # (h2, w2, H, W)
    (3, 4, 9, 9), (13, 17, 50, 70),
    (5, 7, 7, 9),                # identity on the padded grid
    (12, 16, 6, 8),              # downsampling
    (4, 5, 1, 9), (4, 5, 9, 1),  # sy == 0 / sx == 0: every output reads the ring
    (1, 1, 8, 8), (2, 3, 40, 60),            # 10x and more: span 1 / sy + 2
]
BILINEAR_CASES = [               # (h, w, oh, ow, C)
    (5, 7, 9, 13, 4), (7, 7, 7, 7, 3),
    (24, 32, 6, 8, 3),           # downsampling by 4
    (9, 13, 5, 7, 2),            # non-integer downsampling
    (1, 1, 6, 5, 2), (6, 5, 1, 1, 2),
    (2, 3, 31, 47, 1),           # 15x: window ceil((iy + 1) / ry) + 1
    (12, 16, 24, 32, 2),
]
BILINEAR_EXACT_CASES = [(6, 8, 12, 16, 2), (6, 8, 24, 32, 4)]            # integer up-ratios: dyadic weights, integer gradients, exact sums
BILINEAR_B = 2


def bilinear_case(h, w, oh, ow, C):
    """Random gradient [2, oh, ow, C] and prior [2, h, w, C] of one bounded case (float32)."""
    rng = np.random.default_rng(9000 + 100 * h + oh + C)
    return rng.standard_normal((BILINEAR_B, oh, ow, C)).astype(F32), rng.standard_normal((BILINEAR_B, h, w, C)).astype(F32)


def bilinear_errors(got, dout, h, w, gain=1.0, prior=None):
    want = resize_bilinear_backward_ref(dout, h, w, gain, prior, F64)
    unit = resize_bilinear_backward_units(dout, h, w, gain, prior)
    got = np.asarray(got, F64)
    e = np.where(unit > 0, np.abs(got - want) / np.where(unit > 0, unit, 1.0), np.where(got == want, 0.0, np.inf))
    return float(np.where(np.isfinite(got), e, np.inf).max())


# Largest error of the float32 restatement over BILINEAR_CASES (gain 1, and gain 2 accumulated onto a prior), in units; measured
# (tests/test_train_kernels_ref_cpu.py::test_bilinear_fp32_restatement_sets_the_bound) 2.3250
BILINEAR_FP32_UNITS = 2.33
BILINEAR_BOUND = GPU_FACTOR * BILINEAR_FP32_UNITS


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()
