"""Gradients of the 3-D volume transformer on the GPU (vstab_st3d_transform_backward, vstab_st3d_bilinear_interp_backward, the
autograd Functions of spatial_transformer.py) against tests/st3d_ref.py: fp64 autograd on the kernels' own fp32 coordinates, so
every floor and clip decision is shared and every element is compared.

Tolerances have the form (n + r) eps S of tests/test_gpu_st_backward.py, eps = 2^-24, with the reference's count n and absolute
companion S per element (st3d_ref's docstring) and r counted from the sequence sampler3d_ops.hip evaluates, one per fp32 operation,
each rounding a quantity the companion bounds:
  d vol        (n + 3) eps S.  The weight factors x1f - x etc. are exact in fp32; two roundings for the weight (wz * wy) * wx, one
               for w * dout, at most n - 1 for a sum of n terms in any order (the atomics' arrival order).  With accumulate = 1
               the prior value p is one more term: (n + 4) eps (S + |p|).
  d x, d y, d z  (r + C) eps S with r = 17: one channel's term (st3_slope) is four tap differences, four pair weights (wz * wy),
               four products, three sums and the product with dout = 16 operations; the channel sum adds at most C - 1; the
               chain factor (n - 1) / 2 (exact) costs one product.
  d theta      (r' + C) eps S with r' = 18: the per-voxel gx, gy, gz above; their products with x_t, y_t, z_t and the sum over
               voxels are taken in double (2^-53: nothing at this scale); one rounding of the sum to fp32."""
import math

import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime, spatial_transformer as st, training
from tests import st3d_ref as ref
from tests.test_gpu_st3d import IDENTITY, NEAR_IDENTITY, OUT, VOL, affine3, special_coords

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
R_VOL, R_COORD, R_THETA = 3, 17, 18

THETAS = {
    "near_identity": NEAR_IDENTITY,
    # zoom out by 3: the grid covers 27 x the volume, most of it outside -- clip and pad
    "scale3": torch.stack([affine3(30.0, 10.0, -40.0, 3.0, (0.2, -0.3, 0.1)), affine3(0.0, 0.0, 0.0, 3.0, (0.0, 0.0, 0.0))]),
    # zoom in by 3: many output voxels add into each source voxel
    "zoom_in": torch.stack([affine3(25.0, -35.0, 50.0, 0.33, (0.1, 0.05, -0.1)), affine3(-10.0, 5.0, 3.0, 0.3, (0.3, -0.2, 0.0))]),
}


def _check(name, got, want, bound):
    got, want, bound = got.detach().cpu().double().reshape(-1), want.reshape(-1), bound.reshape(-1)
    ok = torch.isfinite(want) & torch.isfinite(bound)
    assert torch.isfinite(got[torch.isfinite(want)]).all(), f"{name}: not finite where the reference is"
    err = (got - want).abs()[ok]
    over = err > bound[ok]
    worst = float((err / bound[ok].clamp_min(1e-300))[bound[ok] > 0].max()) if (bound[ok] > 0).any() else 0.0
    print(f"{name}: max |err| {float(err.max()) if err.numel() else 0.0:.3e}, worst err / bound {worst:.3f}, elements {int(ok.sum())}")
    assert not over.any(), f"{name}: {int(over.sum())} elements over the bound, worst err / bound {worst:.3f}"


def _case(C_, seed, dims=VOL, out=OUT, B=2):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, *dims, C_, generator=g), torch.randn(B, *out, C_, generator=g)


@pytest.mark.parametrize("name", ["near_identity", "scale3", "zoom_in"])
@pytest.mark.parametrize("C_", [1, 2, 3, 4])
def test_transform_backward_matches_reference(name, C_):
    vol, dout = _case(C_, 10 * C_ + 3)
    theta = THETAS[name]
    s, leaves = ref.grad_transform(vol, theta, OUT)
    r = ref.backward(s, leaves, dout)
    d_vol, d_theta = training.st3d_transform_backward(vol.cuda(), theta.cuda(), dout.cuda(), OUT)
    again = training.st3d_transform_backward(vol.cuda(), theta.cuda(), dout.cuda(), OUT)[1]
    _check(f"d_vol[{name},C={C_}]", d_vol, r["d_vol"], (r["n_vol"] + R_VOL) * EPS * r["S_vol"])
    _check(f"d_theta[{name},C={C_}]", d_theta, r["d_theta"], (R_THETA + C_) * EPS * r["S_theta"])
    assert d_theta.shape == (2, 12) and d_vol.shape == vol.shape
    assert torch.equal(d_theta, again)                                         # reproducible: no atomics in this sum


@pytest.mark.parametrize("dims,out", [((1, 7, 9), OUT), (VOL, (1, OUT[1], OUT[2]))])
def test_transform_backward_flat_volume_and_flat_output(dims, out):
    vol, dout = _case(2, 5, dims, out)
    s, leaves = ref.grad_transform(vol, NEAR_IDENTITY, out)
    r = ref.backward(s, leaves, dout)
    d_vol, d_theta = training.st3d_transform_backward(vol.cuda(), NEAR_IDENTITY.cuda(), dout.cuda(), out)
    _check("d_vol", d_vol, r["d_vol"], (r["n_vol"] + R_VOL) * EPS * r["S_vol"])
    _check("d_theta", d_theta, r["d_theta"], (R_THETA + 2) * EPS * r["S_theta"])


@pytest.mark.parametrize("edge", [0, 1, 2])
@pytest.mark.parametrize("C_", [1, 4])
def test_bilinear_interp3d_backward_matches_reference(edge, C_):
    g = torch.Generator().manual_seed(100 + C_ + edge)
    vol = torch.rand(2, *VOL, C_, generator=g)
    n = 2 * OUT[0] * OUT[1] * OUT[2]
    x, k = special_coords(n, g)
    y, z = special_coords(n, g)[0].roll(1), special_coords(n, g)[0].roll(2)
    dout = torch.randn(n, C_, generator=g)
    s, leaves = ref.grad_bilinear_interp3d(vol, x, y, z, OUT, edge)
    r = ref.backward(s, leaves, dout)
    args = (vol.cuda(), x.cuda(), y.cuda(), z.cuda(), dout.cuda(), OUT)
    d_vol, d_x, d_y, d_z = training.st3d_bilinear_interp_backward(*args, edge_size=edge)
    for nm, got in (("x", d_x), ("y", d_y), ("z", d_z)):
        _check(f"d_{nm}[C={C_},e={edge}]", got, r["d_" + nm], (R_COORD + C_) * EPS * r["S_" + nm])
    _check(f"d_vol[C={C_},e={edge}]", d_vol, r["d_vol"], (r["n_vol"] + R_VOL) * EPS * r["S_vol"])
    assert float(d_x[6]) == 0.0 and float(d_y[7]) == 0.0 and float(d_z[8]) == 0.0            # NaN coordinates get no gradient
    # each nullable output in turn; d x, d y, d z are reproducible
    a = training.st3d_bilinear_interp_backward(*args, edge_size=edge, need_vol=False)
    assert a[0] is None and torch.equal(a[1], d_x) and torch.equal(a[2], d_y) and torch.equal(a[3], d_z)
    b = training.st3d_bilinear_interp_backward(*args, edge_size=edge, need_x=False, need_z=False)
    assert b[1] is None and b[3] is None and torch.equal(b[2], d_y)
    c = training.st3d_bilinear_interp_backward(*args, edge_size=edge, need_x=False, need_y=False, need_z=False)
    assert c[1] is None and c[2] is None and c[3] is None
    _check("d_vol alone", c[0], r["d_vol"], (r["n_vol"] + R_VOL) * EPS * r["S_vol"])


def test_d_vol_accumulates_and_null_outputs_skip_their_work():
    C_ = 3
    vol, dout = _case(C_, 77)
    theta = THETAS["near_identity"]
    s, leaves = ref.grad_transform(vol, theta, OUT)
    r = ref.backward(s, leaves, dout)
    volc, thc, dc = vol.cuda(), theta.cuda(), dout.cuda()
    both_vol, both_theta = training.st3d_transform_backward(volc, thc, dc, OUT)
    only_vol, none_theta = training.st3d_transform_backward(volc, thc, dc, OUT, need_theta=False)
    none_vol, only_theta = training.st3d_transform_backward(volc, thc, dc, OUT, need_vol=False)
    assert none_theta is None and none_vol is None
    assert torch.equal(only_theta, both_theta)                                # the same sum in the same order
    _check("d_vol alone", only_vol, r["d_vol"], (r["n_vol"] + R_VOL) * EPS * r["S_vol"])
    prior = torch.randn(vol.shape, generator=torch.Generator().manual_seed(5))
    acc = prior.clone().cuda()
    got, _ = training.st3d_transform_backward(volc, thc, dc, OUT, need_theta=False, d_vol=acc)
    assert got.data_ptr() == acc.data_ptr()
    _check("d_vol accumulated", acc, prior.double() + r["d_vol"], (r["n_vol"] + R_VOL + 1) * EPS * (r["S_vol"] + prior.double().abs()))
    # through the ABI: accumulate = 0 overwrites whatever was there, NaN included; a NULL d_theta needs no workspace; a NULL d_vol
    # leaves the buffer it would have written alone
    L = _lib.lib()
    sp = runtime.stream_ptr()
    buf = torch.full(vol.shape, float("nan"), device="cuda")
    shape = (2, *VOL, C_)
    assert L.vstab_st3d_transform_backward(volc.data_ptr(), *shape, thc.data_ptr(), dc.data_ptr(), *OUT, buf.data_ptr(), 0, None, None, 0, sp) == 0
    _check("d_vol over NaN", buf, r["d_vol"], (r["n_vol"] + R_VOL) * EPS * r["S_vol"])
    need = L.vstab_st3d_transform_backward_workspace_bytes(*shape, *OUT)
    assert need > 0 and need % 8 == 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    d_th = torch.full((2, 12), 7.0, device="cuda")
    assert L.vstab_st3d_transform_backward(volc.data_ptr(), *shape, thc.data_ptr(), dc.data_ptr(), *OUT, None, 0, d_th.data_ptr(), ws.data_ptr(), need, sp) == 0
    assert torch.equal(d_th, both_theta)
    assert L.vstab_st3d_transform_backward(volc.data_ptr(), *shape, thc.data_ptr(), dc.data_ptr(), *OUT, None, 0, d_th.data_ptr(), ws.data_ptr(), need - 8, sp) == -4
    assert L.vstab_st3d_transform_backward(volc.data_ptr(), *shape, thc.data_ptr(), dc.data_ptr(), *OUT, None, 0, None, None, 0, sp) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- autograd
def test_autograd_through_transform_is_the_explicit_backward():
    vol, dout = _case(2, 31)
    theta = THETAS["near_identity"]
    volc, thc = vol.cuda().requires_grad_(True), theta.cuda().requires_grad_(True)
    tr = st.AffineVolumeTransformer(OUT)
    y = tr.transform(volc, thc)
    assert y.grad_fn is not None and y.shape == (2, *OUT, 2)
    g_vol, g_th = torch.autograd.grad(y, (volc, thc), dout.cuda())
    e_vol, e_th = training.st3d_transform_backward(vol.cuda(), theta.cuda(), dout.cuda(), OUT)
    assert g_th.shape == theta.shape and torch.equal(g_th, e_th)
    s, leaves = ref.grad_transform(vol, theta, OUT)
    r = ref.backward(s, leaves, dout)
    _check("autograd d_vol", g_vol, r["d_vol"], (r["n_vol"] + R_VOL) * EPS * r["S_vol"])
    plain = tr.transform(vol.cuda(), theta.cuda())
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, y.detach())
    with torch.no_grad():
        assert tr.transform(volc, thc).grad_fn is None


def test_autograd_frozen_volume_or_frozen_theta_skips_that_gradient(monkeypatch):
    vol, dout = _case(1, 32)
    theta = THETAS["near_identity"]
    calls = []
    real = training.st3d_transform_backward

    def spy(*a, **k):
        calls.append((k["need_vol"], k["need_theta"]))
        res = real(*a, **k)
        calls.append(tuple(t is not None for t in res))
        return res

    monkeypatch.setattr(training, "st3d_transform_backward", spy)
    tr = st.AffineVolumeTransformer(OUT)
    volc = vol.cuda().requires_grad_(True)
    (g_vol,) = torch.autograd.grad(tr.transform(volc, theta.cuda()), (volc,), dout.cuda())
    assert calls == [(True, False), (True, False)]                       # the d theta reduction is not launched
    calls.clear()
    thc = theta.cuda().requires_grad_(True)
    (g_th,) = torch.autograd.grad(tr.transform(vol.cuda(), thc), (thc,), dout.cuda())
    assert calls == [(False, True), (False, True)]                       # a frozen volume costs no scatter
    assert torch.equal(g_th, real(vol.cuda(), theta.cuda(), dout.cuda(), OUT, need_vol=False)[1])


def test_autograd_through_bilinear_interp3d_is_the_explicit_backward(monkeypatch):
    g = torch.Generator().manual_seed(8)
    C_, edge = 2, 2
    vol = torch.rand(2, *VOL, C_, generator=g)
    n = 2 * OUT[0] * OUT[1] * OUT[2]
    x, y, z = (torch.rand(n, generator=g) * 2.4 - 1.2 for _ in range(3))
    dout = torch.randn(n, C_, generator=g)
    volc = vol.cuda().requires_grad_(True)
    xc, yc, zc = (t.cuda().requires_grad_(True) for t in (x, y, z))
    out = st.bilinear_interp3d(volc, xc, yc, zc, OUT, edge_size=edge)
    assert out.grad_fn is not None
    g_vol, g_x, g_y, g_z = torch.autograd.grad(out, (volc, xc, yc, zc), dout.cuda())
    e = training.st3d_bilinear_interp_backward(vol.cuda(), x.cuda(), y.cuda(), z.cuda(), dout.cuda(), OUT, edge_size=edge)
    assert torch.equal(g_x, e[1]) and torch.equal(g_y, e[2]) and torch.equal(g_z, e[3])
    s, leaves = ref.grad_bilinear_interp3d(vol, x, y, z, OUT, edge)
    r = ref.backward(s, leaves, dout)
    _check("autograd d_vol", g_vol, r["d_vol"], (r["n_vol"] + R_VOL) * EPS * r["S_vol"])
    plain = st.bilinear_interp3d(vol.cuda(), x.cuda(), y.cuda(), z.cuda(), OUT, edge_size=edge)
    assert plain.grad_fn is None and torch.equal(plain, out.detach())
    # only z asks for a gradient: only its kernel work is requested
    seen = []
    real = training.st3d_bilinear_interp_backward
    monkeypatch.setattr(training, "st3d_bilinear_interp_backward",
                        lambda *a, **k: (seen.append((k["need_vol"], k["need_x"], k["need_y"], k["need_z"])), real(*a, **k))[1])
    (only_z,) = torch.autograd.grad(st.bilinear_interp3d(vol.cuda(), x.cuda(), y.cuda(), zc, OUT, edge_size=edge), (zc,), dout.cuda())
    assert seen == [(False, False, False, True)] and torch.equal(only_z, g_z)


# ------------------------------------------------------------------------------------------------------ gradient descent
GD_DIMS, GD_STEP, GD_STEPS = (12, 16, 20), 0.2, 40
GD_TARGET = affine3(3.0, -2.0, 4.0, 1.03, (0.04, -0.03, 0.02))


def smooth_volume(dims=GD_DIMS):
    z, y, x = torch.meshgrid(*(torch.linspace(0, 1, n) for n in dims), indexing='ij')
    v = 0.5 + 0.2 * torch.sin(2 * math.pi * (1.0 * x + 0.5 * y + 0.3 * z)) + 0.15 * torch.cos(2 * math.pi * (0.7 * y - 0.4 * x + 0.6 * z)) \
        + 0.15 * torch.sin(2 * math.pi * (0.8 * z - 0.5 * y) + 1.0)
    return v.reshape(1, *dims, 1).float()


def descend(transform, vol, target_theta, theta0):
    """plain SGD on the MSE between transform(vol, theta) and transform(vol, theta*): (first loss, last loss, theta)"""
    target = transform(vol, target_theta).detach()
    theta = theta0.clone().requires_grad_(True)
    first = None
    for _ in range(GD_STEPS):
        loss = ((transform(vol, theta) - target) ** 2).mean()
        (g,) = torch.autograd.grad(loss, theta)
        first = float(loss.detach()) if first is None else first
        theta = (theta.detach() - GD_STEP * g).requires_grad_(True)
    final = float(((transform(vol, theta.detach()) - target) ** 2).mean())
    return first, final, theta.detach()


def reference_transform(vol, theta):
    """st3d_ref's graph as a differentiable function of theta (fp64 autograd, fp32 decisions)"""
    s, (vol64, th) = ref.grad_transform(vol, theta.detach().reshape(1, 12), GD_DIMS)

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return s.out.detach().clone()

        @staticmethod
        def backward(ctx, dout):
            return torch.autograd.grad(s.out, th, dout)[0].reshape(t_shape).to(theta.dtype)

    t_shape = theta.shape
    return Fn.apply(theta)


def test_gradient_descent_recovers_a_known_affine_theta():
    """theta* = rotations (3, -2, 4) degrees, 3 % zoom, shift (0.04, -0.03, 0.02), recovered from the identity by plain gradient
    descent (step GD_STEP, GD_STEPS steps) on the MSE between transform(vol, theta) and transform(vol, theta*), on a
    12 x 16 x 20 x 1 volume of a few low-frequency sinusoids.  The same loop on the CPU through tests/st3d_ref.py (fp64 autograd
    on the fp32 decisions; `python -m tests.test_gpu_st3d_backward` prints it) brings the loss to CPU_RATIO = 2.034e-4 of its start
    (2.6031e-02 -> 5.2952e-06); the GPU
    loop differs only by fp32 rounding of a smooth loss, and has to reach that ratio within a factor 10."""
    vol = smooth_volume()
    tr = st.AffineVolumeTransformer(GD_DIMS)
    first, final, theta = descend(lambda v, t: tr.transform(v, t), vol.cuda(), GD_TARGET.reshape(1, 12).cuda(), IDENTITY.reshape(1, 12).cuda())
    print(f"loss {first:.4e} -> {final:.4e} (ratio {final / first:.3e}, reference {CPU_RATIO:.3e}); theta {theta.cpu().tolist()}")
    assert final / first <= 10 * CPU_RATIO


CPU_RATIO = 2.034e-4          # the CPU loop below: loss 2.6031e-02 -> 5.2952e-06


if __name__ == "__main__":
    f0, f1, th = descend(reference_transform, smooth_volume(), GD_TARGET.reshape(1, 12).double(), IDENTITY.reshape(1, 12).double())
    print(f"reference loop: loss {f0:.4e} -> {f1:.4e}, ratio {f1 / f0:.3e}; theta {th.tolist()}")
