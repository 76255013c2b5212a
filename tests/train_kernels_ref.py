"""Plain references for three kernels of the training step, one entry point each: `vstab_column_sum` (bias gradients, flow-head
sums), `vstab_pf2_taps_backward` (the adjoint of the full-resolution head's tap gather, model.py:882-885) and `vstab_adam_step`
(tf.train.AdamOptimizer, main:333-335).  tests/test_train_kernels_ref_cpu.py anchors them to independent statements on the CPU,
tests/test_gpu_train_kernels.py compares the kernels with them.

The column sum and the gather adjoint are compared EXACTLY: their test inputs are small integers held in float32, every partial sum
stays below 2^24, so float addition is exact in any order and the fp64 reference cast to float32 is the only right answer.

Adam is compared within a bound measured here.  `adam_ref(dtype=np.float64)` is the reference; `adam_ref(dtype=np.float32)` restates
the kernel's statement sequence with one IEEE rounding per operation (the library is built with -ffp-contract=off).  The error of
each of w, m, v is expressed in UNITS of

    2^-24 * (sum of the absolute values of the terms added) + 2^-149

    m:  |b1 m| + |(1-b1) g|        v:  |b2 v| + |(1-b2) g^2|        w:  |w| + |lr_t m / (sqrt(v) + eps)|

The 2^-149 is one step of float32's subnormal range: below 2^-126 a float32 rounding error is absolute, not relative, and the planted
|g| = 1e-20 puts (1-b2) g^2 = 1e-43 there (it does not vanish: it is 71 subnormal steps, known to 0.7 %).  Without that term the unit
of v at that element would be 6e-51 and the float32 restatement itself would sit 1e5 units away from the fp64 value; everywhere else
the term is at least 2^-100 times smaller than the rest of the unit.

ADAM_FP32_UNITS are the largest errors of the float32 restatement over every case of `ADAM_CASES` and the four steps of each,
measured by tests/test_train_kernels_ref_cpu.py (which fails when they no longer hold); the GPU may use ADAM_GPU_FACTOR = 4 times as
much, for a device square root and division that need not be correctly rounded."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import vstab_oracle as vo

EPS32 = 2.0 ** -24
TINY32 = 2.0 ** -149


# ----------------------------------------------------------------------------- column sum
def column_sum_ref(g, c_off, C):
    """out[c] = sum over every leading axis of g[..., c_off + c], in fp64."""
    g = torch.as_tensor(g)
    return g[..., c_off:c_off + C].double().reshape(-1, C).sum(dim=0)


# ----------------------------------------------------------------------------- full-resolution head: the tap gather and its adjoint
def tap_table(concat2, W_hwio):
    """T[n,y,x,2*tap+o] = sum_c concat2[n,y,x,c] W[dy,dx,c,o], tap = 3*dy + dx: the 3x3 head applied per SOURCE pixel, 18 of the 32
    columns used (include/vstab.h, vstab_predict2_tap_table)."""
    B, h2, w2, Cin = concat2.shape
    T = torch.zeros(B, h2, w2, 32, dtype=concat2.dtype)
    T[..., :18] = torch.einsum("nyxc,tco->nyxto", concat2, W_hwio.reshape(9, Cin, 2).to(concat2.dtype)).reshape(B, h2, w2, 18)
    return T


def pf2_tap_gather(T, H, W):
    """The linear part of the full-resolution head, in the dtype of T [B,h2,w2,32]:
    out[n,y,x,o] = sum_tap Tpad[n, iy[y+dy], ix[x+dx], 2*tap+o] for y < H-2, x < W-2, Tpad = T inside a ring of zeros, iy / ix the
    nearest-neighbour (align_corners) maps of the padded grid to H and W.  No bias, no predict_flow3."""
    B, h2, w2, _ = T.shape
    iy = torch.from_numpy(vo.nearest_align_corners_index(h2 + 2, H))
    ix = torch.from_numpy(vo.nearest_align_corners_index(w2 + 2, W))
    Tp = F.pad(T, (0, 0, 1, 1, 1, 1))
    oh, ow = H - 2, W - 2
    out = torch.zeros(B, oh, ow, 2, dtype=T.dtype)
    for dy in range(3):
        for dx in range(3):
            tap = 3 * dy + dx
            out = out + Tp[:, iy[dy:dy + oh]][:, :, ix[dx:dx + ow]][..., 2 * tap:2 * tap + 2]
    return out


def pf2_taps_backward_ref(g, h2, w2, H, W):
    """dT [B,h2,w2,32] (fp64, columns 18..31 zero) = the adjoint of `pf2_tap_gather` applied to g [B,H-2,W-2,2], by autograd."""
    g = torch.as_tensor(g).double()
    T = torch.zeros(g.shape[0], h2, w2, 32, dtype=torch.float64, requires_grad=True)
    pf2_tap_gather(T, H, W).backward(g)
    return T.grad.detach()


# (B, h2, w2, H, W, cs_g) of the GPU test; the CPU test proves the adjoint identity of the reference at the same shapes
PF2_CASES = [
    (1, 1, 1, 3, 3, 2),          # smallest: one source pixel, one output pixel, all nine taps on it or on the ring
    (2, 5, 7, 7, 9, 4),          # H = h2 + 2: the identity map of the coarse heads
    (2, 24, 32, 96, 128, 4),     # the network's ratio
    (1, 13, 17, 50, 66, 2),      # odd sizes, ragged tiles
    (1, 3, 4, 40, 9, 4),         # about ten output rows per source row in y, a shrinking ratio in x
    (1, 64, 64, 34, 34, 4),      # downsampling: most source pixels receive nothing
    (2, 40, 90, 20, 70, 2),
]


# ----------------------------------------------------------------------------- Adam
def lr_t(lr, b1, b2, t):
    """The step size the caller hands to the kernel: lr sqrt(1 - b2^t) / (1 - b1^t)."""
    return lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def _hyper(dtype, *values):
    return [dtype(np.float32(x)) for x in values]      # the kernel receives floats


def adam_ref(w, g, m, v, lr_t, b1, b2, eps, dtype=np.float64):
    """One TF-style step, m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2; w -= lr_t m / (sqrt(v) + eps), returned as (w, m, v) in `dtype`.
    np.float64 is the reference.  np.float32 is the kernel's own sequence, `b1 * m + (1.f - b1) * g`, `b2 * v + (1.f - b2) * g * g`
    (left to right) and `w - lr_t * m / (sqrtf(v) + eps)`, with one rounding per operation."""
    lr_t, b1, b2, eps = _hyper(dtype, lr_t, b1, b2, eps)
    w, g, m, v = (np.asarray(a).astype(dtype) for a in (w, g, m, v))
    one = dtype(1.0)
    m = b1 * m + (one - b1) * g
    v = b2 * v + (one - b2) * g * g
    w = w - lr_t * m / (np.sqrt(v) + eps)
    return w, m, v


def adam_units(w, g, m, v, lr_t, b1, b2, eps):
    """The units (module docstring) of the errors of w, m and v after one step from the state (w, m, v): three fp64 arrays."""
    lr_t, b1, b2, eps = _hyper(np.float64, lr_t, b1, b2, eps)
    w, g, m, v = (np.asarray(a).astype(np.float64) for a in (w, g, m, v))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    um = np.abs(b1 * m) + np.abs((1.0 - b1) * g)
    uv = np.abs(b2 * v) + np.abs((1.0 - b2) * g * g)
    uw = np.abs(w) + np.abs(lr_t * m1 / (np.sqrt(v1) + eps))
    return tuple(EPS32 * u + TINY32 for u in (uw, um, uv))


def adam_errors(got, state, g, lr_t, b1, b2, eps):
    """Largest error of `got` = (w, m, v) after one step from `state` = (w, m, v) with gradient g, against the fp64 reference, in
    units: (err_w, err_m, err_v).  Anything not finite counts as infinitely wrong."""
    want = adam_ref(*([state[0], g, state[1], state[2]]), lr_t, b1, b2, eps, dtype=np.float64)
    units = adam_units(state[0], g, state[1], state[2], lr_t, b1, b2, eps)
    out = []
    for a, r, u in zip(got, want, units):
        a = np.asarray(a).astype(np.float64)
        e = np.abs(a - r) / u
        out.append(float(np.where(np.isfinite(a), e, np.inf).max()))
    return tuple(out)


ADAM_LR, ADAM_B2, ADAM_EPS, ADAM_STEPS = 1e-3, 0.999, 1e-8, 4
ADAM_CASES = [(1, 0.9), (255, 0.9), (256, 0.9), (257, 0.9), (100003, 0.9), (257, 0.5)]        # (n, beta1); 0.5 is what main passes
# planted elements (those that fit into n): index -> what it is
ADAM_PLANT = {3: "g = 0, m != 0", 17: "g = m = v = 0", 101: "|g| = 1e4", 200: "|g| = 1e-20, v = 0"}


def adam_case(n, b1):
    """State and gradients of one GPU test case: float32 arrays w, m (non-zero), v (>= 0, non-zero) of n elements and g [4, n], one
    gradient per step; the planted elements of ADAM_PLANT keep their g at every step."""
    rng = np.random.default_rng(1000 + n + int(b1 * 10))
    w = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.1).astype(np.float32)
    v = (rng.standard_normal(n) ** 2 * 0.01 + 1e-4).astype(np.float32)
    g = (rng.standard_normal((ADAM_STEPS, n)) * 0.1).astype(np.float32)
    if n > 3:
        g[:, 3], m[3] = 0.0, 0.25
    if n > 17:
        g[:, 17], m[17], v[17] = 0.0, 0.0, 0.0
    if n > 101:
        g[:, 101] = np.float32(1e4) * np.array([1, -1, 1, 1], np.float32)
    if n > 200:
        g[:, 200], m[200], v[200] = np.float32(1e-20) * np.array([1, 1, -1, 1], np.float32), -0.5, 0.0
    return w, m, v, g


# Largest error of the float32 restatement, in units, of (w, m, v) over ADAM_CASES x 4 steps, each step taken from the restatement's
# own previous state (w's is at an element with |w| = 7e-6 next to a step of 1e-4 whose m is a difference of two terms): measured 3.2963, 1.8750, 1.9591 (tests/test_train_kernels_ref_cpu.py::test_adam_fp32_restatement_sets_the_bound)
ADAM_FP32_UNITS = (3.30, 1.88, 1.96)
ADAM_GPU_FACTOR = 4.0
ADAM_BOUND = tuple(ADAM_GPU_FACTOR * u for u in ADAM_FP32_UNITS)
