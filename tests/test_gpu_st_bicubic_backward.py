"""Gradients of the BICUBIC sampler on the GPU (vstab_st_bicubic_interp_backward, the three _interp_backward entry points, the
`differentiable=True` autograd path of spatial_transformer.py) against tests/st_bicubic_grad_ref.py: fp64 autograd on the kernels' own
fp32 coordinates, so every floor, clip and clamp decision is shared and every element is compared.

Tolerances, eps = 2^-24, with the reference's count n and absolute companion S per element (S is built from the weights' absolute
companions |w|_i = sum_k |c_ik| t^k, st_bicubic_grad_ref's docstring).  Roundings counted from csrc/sampler_ops.hip, first order in eps,
plus 1 for the second-order terms; t = v - floor(v) is exact in fp32 and is the reference's own value:
  a weight     cubic_axis: t2 = t t (1), t3 = t2 t (2); ((c0 + c1 t) + c2 t2) + c3 t3 -- the term c1 t carries its product and three
               sums, c2 t2 two + product + two sums, c3 t3 three + product + one sum: 4 eps |w|.  A derivative weight
               (c1 + 2c2 t) + 3c3 t2 (the doubled and tripled coefficients are exact): 3 eps |w'|.
  d img        (n + R_IMG) eps S, R_IMG = 10 + 1: a contribution wx_j * (wy_i * dout) is two weights (4 + 4) and two products;
               at most n - 1 roundings for a sum of n terms in any order (the atomics' arrival order), n counting the replicated
               and folded taps.  With accumulate = 1 the prior value is one more term: (n + R_IMG + 1) eps (S + |prior|).
  d x, d y     (R_COORD + C) eps S, R_COORD = 16 + 1: per channel d_i = ((w'0 I0 + w'1 I1) + w'2 I2) + w'3 I3 is 3 (weight) + 1
               (product) + 3 (sums) = 7; wy_i * d_i adds 4 + 1 = 12; the four rows' sum 3 more = 15; times dout 16; the channel sum
               at most C - 1; the chain factor (n - 1) / 2 (exact) one product: 16 + C.  d y is the same count with the roles of
               w and w' exchanged (4 + 1 + 3, then 3 + 1).
  d theta      (R_COORD + 1 + C) eps S_theta: the per-pixel values above; the products with x_t, y_t, 1 / z, x_h, y_h and the sums are
               taken in double; one rounding of the result to fp32.  SimilarityTransformer 8 more (cosf / sinf within 4 ulp: the
               count of test_gpu_st_sym_backward.py); the spline 9 more (the fp32 U_k: the count of test_gpu_st_tps_backward.py)."""
import functools

import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime, spatial_transformer as st, training
from tests import st_bicubic_grad_ref as ref
from tests import st_sym_grad_ref as sref
from tests.test_gpu_st_backward import EPS, _check, _rot, _smooth_image, _theta

pytestmark = pytest.mark.gpu
R_IMG, R_COORD = 11, 17
R_THETA = R_COORD + 1
BC = 'bicubic'


def _img_bound(r, prior=None):
    if prior is None:
        return (r["n_img"] + R_IMG) * EPS * r["S_img"]
    return (r["n_img"] + R_IMG + 1) * EPS * (r["S_img"] + prior.double().abs())


@functools.lru_cache(maxsize=None)
def _theta_case(name, C_, tdim):
    """One run of the reference and of the device, shared by the tests (nothing in it is modified)."""
    g = torch.Generator().manual_seed(10 * C_ + tdim)
    im, dout, out = torch.rand(2, 40, 52, C_, generator=g), torch.randn(2, 37, 45, C_, generator=g), (37, 45)
    theta = _theta(name, tdim)
    s, leaves = ref.transform(im, theta, out)
    r = ref.backward(s, leaves, dout)
    d_img, d_theta = training.st_transform_backward(im.cuda(), theta.cuda(), dout.cuda(), out, interp=BC)
    return dict(im=im, dout=dout, out=out, theta=theta, r=r, d_img=d_img, d_theta=d_theta)


CASES = [(name, C_, tdim) for name in ("near_identity", "rotation_zoom", "outside") for C_ in (3, 1, 4) for tdim in (6, 8)]
CASES += [("z_cross", C_, 8) for C_ in (3, 1, 4)]


@pytest.mark.parametrize("name,C_,tdim", CASES)
def test_transform_backward_matches_reference(name, C_, tdim):
    """Affine and projective, the tile kernel (C = 3) and the pixel kernel (C = 1, 4), 40 x 52 -> 37 x 45; d theta bit-equal across
    two calls."""
    c = _theta_case(name, C_, tdim)
    _check(f"d_img[{name},C={C_},tdim={tdim}]", c["d_img"], c["r"]["d_img"], _img_bound(c["r"]))
    _check(f"d_theta[{name},C={C_},tdim={tdim}]", c["d_theta"], c["r"]["d_theta"], (R_THETA + C_) * EPS * c["r"]["S_theta"])
    again = training.st_transform_backward(c["im"].cuda(), c["theta"].cuda(), c["dout"].cuda(), c["out"], need_img=False, interp=BC)[1]
    assert c["d_theta"].shape == (2, tdim) and torch.equal(c["d_theta"], again)


def _coords_case(B, C_, H=13, W=17, oh=19, ow=23):
    g = torch.Generator().manual_seed(100 + C_)
    im = torch.rand(B, H, W, C_, generator=g)
    n = B * oh * ow
    x, y = torch.rand(n, generator=g) * 2.6 - 1.3, torch.rand(n, generator=g) * 2.6 - 1.3
    special = torch.tensor([-1.0, 1.0, float("nan"), float("inf"), -float("inf"), 0.0, 1.0 + 2.0 ** -23, -3.0, 7.5, -1.0 - 2.0 ** -23, 0.5])
    x[:special.numel()] = special
    y[:special.numel()] = special.flip(0)
    return im, x, y, torch.randn(n, C_, generator=g), (oh, ow), special


@pytest.mark.parametrize("B,C_", [(1, 1), (2, 3), (2, 4)])
def test_bicubic_interp_backward_matches_reference(B, C_):
    """Explicit coordinates with exact +-1 (full gradient), one ulp beyond, far beyond, inf and NaN (none); each nullable output in
    turn; accumulate; d x, d y reproducible."""
    im, x, y, dout, out, special = _coords_case(B, C_)
    s, leaves = ref.bicubic_interp(im, x, y, out)
    r = ref.backward(s, leaves, dout)
    imc, xc, yc, dc = im.cuda(), x.cuda(), y.cuda(), dout.cuda()
    d_img, d_x, d_y = training.st_bicubic_interp_backward(imc, xc, yc, dc, out)
    _check(f"d_x[C={C_}]", d_x, r["d_x"], (R_COORD + C_) * EPS * r["S_x"])
    _check(f"d_y[C={C_}]", d_y, r["d_y"], (R_COORD + C_) * EPS * r["S_y"])
    _check(f"d_img[C={C_}]", d_img, r["d_img"], _img_bound(r))
    for k in (2, 3, 4, 6, 7, 8, 9):                                              # NaN, +-inf and everything beyond +-1: no gradient
        assert float(d_x[k]) == 0.0 and float(d_y[special.numel() - 1 - k]) == 0.0
    assert float(r["S_x"][0]) > 0 and float(r["S_x"][1]) > 0                     # exactly +-1 passes
    a = training.st_bicubic_interp_backward(imc, xc, yc, dc, out, need_img=False)
    assert a[0] is None and torch.equal(a[1], d_x) and torch.equal(a[2], d_y)
    b = training.st_bicubic_interp_backward(imc, xc, yc, dc, out, need_x=False)
    assert b[1] is None and torch.equal(b[2], d_y)
    c = training.st_bicubic_interp_backward(imc, xc, yc, dc, out, need_y=False, need_x=False)
    assert c[1] is None and c[2] is None
    _check("d_img alone", c[0], r["d_img"], _img_bound(r))
    prior = torch.randn(im.shape, generator=torch.Generator().manual_seed(5))
    acc = prior.clone().cuda()
    got = training.st_bicubic_interp_backward(imc, xc, yc, dc, out, need_x=False, need_y=False, d_img=acc)[0]
    assert got.data_ptr() == acc.data_ptr()
    _check("d_img accumulated", acc, prior.double() + r["d_img"], _img_bound(r, prior))
    buf = torch.full(im.shape, float("nan"), device="cuda")                       # accumulate = 0 overwrites, NaN included
    assert _lib.lib().vstab_st_bicubic_interp_backward(imc.data_ptr(), B, 13, 17, C_, xc.data_ptr(), yc.data_ptr(), dc.data_ptr(), out[0], out[1],
                                                       buf.data_ptr(), 0, None, None, runtime.stream_ptr()) == 0
    _check("d_img over NaN", buf, r["d_img"], _img_bound(r))


@pytest.mark.parametrize("H,W,C_", [(1, 1, 3), (2, 3, 1), (3, 2, 3), (1, 5, 4), (3, 3, 3)])
def test_edge_folding_conserves_the_gradient(H, W, C_):
    """The smallest images: most of the 16 taps replicate onto few pixels and all of them add.  sum w = 1 on each axis, so per
    channel sum(d img) = sum over the pixels of dout, within the sum of the per-element bounds."""
    B, oh, ow = 2, 6, 7
    g = torch.Generator().manual_seed(H * 10 + W)
    im = torch.rand(B, H, W, C_, generator=g)
    x, y = torch.rand(B * oh * ow, generator=g) * 2.4 - 1.2, torch.rand(B * oh * ow, generator=g) * 2.4 - 1.2
    dout = torch.randn(B * oh * ow, C_, generator=g)
    s, leaves = ref.bicubic_interp(im, x, y, (oh, ow))
    r = ref.backward(s, leaves, dout)
    d_img, d_x, d_y = training.st_bicubic_interp_backward(im.cuda(), x.cuda(), y.cuda(), dout.cuda(), (oh, ow))
    _check(f"d_img[{H}x{W}]", d_img, r["d_img"], _img_bound(r))
    _check(f"d_x[{H}x{W}]", d_x, r["d_x"], (R_COORD + C_) * EPS * r["S_x"])
    _check(f"d_y[{H}x{W}]", d_y, r["d_y"], (R_COORD + C_) * EPS * r["S_y"])
    assert float(r["n_img"].sum()) == 16.0 * B * oh * ow * C_                     # every tap of every point landed on some pixel
    total = d_img.double().cpu().reshape(B, -1, C_).sum(1)
    want = dout.double().reshape(B, -1, C_).sum(1)
    bound = _img_bound(r).reshape(B, -1, C_).sum(1) + 2 * EPS * r["S_img"].reshape(B, -1, C_).sum(1)
    assert bool(((total - want).abs() <= bound).all())


SYM_B, SYM_H, SYM_W = 2, 104, 117                                              # test_gpu_st_sym_backward.py's image and output sizes
SYM_CLS = {'affine': st.AffineSymmetryTransformer, 'projective': st.ProjectiveSymmetryTransformer, 'similarity': st.SimilarityTransformer}
SYM_THETA = {
    'affine': [[0.3, -0.7, 0.2, 0.5, 0.9, -0.4], [-1.1, 0.6, 0.8, -0.2, 0.4, 0.1]],
    'projective': {(24, 40): [[-1115.0, 583.0, -37.0, -392.0, 400.0, 39.0, -15.0, -1.0], [696.0, 1116.0, 25.0, 961.0, -596.0, -37.0, 9.0, 17.0]],
                   (40, 260): [[10.0, -20.0, 30.0, 15.0, 60.0, 40.0, 5.0, -15.0], [-12.0, 25.0, -35.0, -20.0, 80.0, -40.0, -8.0, 12.0]]},
    'similarity': {(24, 40): [[-2.3, 0.4, -0.6, 4.3], [-4.6, 2.3, 1.1, -4.7]], (40, 260): [[1.6, -2.9, 2.8, -4.3], [-4.7, -1.2, 3.7, -3.7]]},
}


@functools.lru_cache(maxsize=None)
def _sym_case(kind, out, C_):
    oh, ow = out
    g = torch.Generator().manual_seed(1000 * C_ + 10 * oh + len(kind))
    im, dout = torch.rand(SYM_B, SYM_H, SYM_W, C_, generator=g), torch.randn(SYM_B, ow, oh, C_, generator=g)
    th = SYM_THETA[kind]
    theta = torch.tensor(th if kind == 'affine' else th[out])
    tr = SYM_CLS[kind](out, interp_method=BC)
    M = tr.matrix(theta.cuda())
    xs, ys = tr.transform_coords(theta.cuda())
    s, leaves = ref.symmetry_transform(kind, im, theta, out, M32=M.cpu(), xs32=xs.cpu(), ys32=ys.cpu())
    r = ref.backward(s, leaves, dout)
    d_img, d_theta = training.st_symmetry_transform_backward(im.cuda(), theta.cuda(), dout.cuda(), out, sref.KIND[kind], interp=BC)
    return dict(im=im, dout=dout, theta=theta, r=r, d_img=d_img, d_theta=d_theta)


@pytest.mark.parametrize("kind,out,C_", [(k, o, c) for k in SYM_CLS for o in ((24, 40), (40, 260)) for c in (3, 1, 4)])
def test_symmetry_backward_matches_reference(kind, out, C_):
    """The thetas of test_gpu_st_sym_backward.py that carry a quarter to a half of the kept pixels beyond the mirrored border: here
    the clip holds them at the padded extent's edge with no gradient.  d theta bit-equal across two calls."""
    c = _sym_case(kind, out, C_)
    r_theta = R_THETA + (8 if kind == 'similarity' else 0)
    _check(f"d_img[{kind},{out},C={C_}]", c["d_img"], c["r"]["d_img"], _img_bound(c["r"]))
    _check(f"d_theta[{kind},{out},C={C_}]", c["d_theta"], c["r"]["d_theta"], (r_theta + C_) * EPS * c["r"]["S_theta"])
    again = training.st_symmetry_transform_backward(c["im"].cuda(), c["theta"].cuda(), c["dout"].cuda(), out, sref.KIND[kind], need_img=False,
                                                    interp=BC)[1]
    assert torch.equal(c["d_theta"], again)
    if kind == 'affine':
        assert bool((c["d_theta"] == 0).all())


@functools.lru_cache(maxsize=None)
def _tps_case(g, C_, out):
    gen = torch.Generator().manual_seed(1000 * g + 10 * C_)
    im = torch.rand(2, 48, 64, C_, generator=gen)
    theta = 0.15 * torch.randn(2, 2 * g * g, generator=gen)
    dout = torch.randn(2, out[0], out[1], C_, generator=gen)
    tr = st.ElasticTransformer(out, g, interp_method=BC)
    xs, ys = tr.transform_coords(theta.cuda())
    s, leaves = ref.elastic(im, xs.cpu(), ys.cpu(), g, out)
    r = ref.elastic_backward(s, leaves, dout, g, tr.L_inv.cpu())
    d_img, d_theta = training.st_elastic_transform_backward(im.cuda(), theta.cuda(), dout.cuda(), out, g, tr.L_inv, interp=BC)
    return dict(im=im, dout=dout, theta=theta, tr=tr, r=r, d_img=d_img, d_theta=d_theta)


@pytest.mark.parametrize("g,C_,out", [(2, 3, (40, 56)), (2, 1, (40, 56)), (4, 3, (40, 56)), (4, 4, (40, 56)), (16, 3, (24, 40))])
def test_elastic_backward_matches_reference(g, C_, out):
    c = _tps_case(g, C_, out)
    _check(f"d_img[g={g},C={C_}]", c["d_img"], c["r"]["d_img"], _img_bound(c["r"]))
    _check(f"d_theta[g={g},C={C_}]", c["d_theta"], c["r"]["d_theta"], (R_THETA + 9 + C_) * EPS * c["r"]["S_theta"])
    again = training.st_elastic_transform_backward(c["im"].cuda(), c["theta"].cuda(), c["dout"].cuda(), out, g, c["tr"].L_inv, need_img=False,
                                                   interp=BC)[1]
    assert torch.equal(c["d_theta"], again)


def test_transform_backward_accumulate_and_nullable_outputs():
    c = _theta_case("near_identity", 3, 6)
    im, th, dout, out, r = c["im"].cuda(), c["theta"].cuda(), c["dout"].cuda(), c["out"], c["r"]
    only_img, none_theta = training.st_transform_backward(im, th, dout, out, need_theta=False, interp=BC)
    none_img, only_theta = training.st_transform_backward(im, th, dout, out, need_img=False, interp=BC)
    assert none_theta is None and none_img is None and torch.equal(only_theta, c["d_theta"])
    _check("d_img alone", only_img, r["d_img"], _img_bound(r))
    prior = torch.randn(c["im"].shape, generator=torch.Generator().manual_seed(5))
    acc = prior.clone().cuda()
    training.st_transform_backward(im, th, dout, out, need_theta=False, d_img=acc, interp=BC)
    _check("d_img accumulated", acc, prior.double() + r["d_img"], _img_bound(r, prior))
    buf = torch.full(c["im"].shape, float("nan"), device="cuda")
    assert _lib.lib().vstab_st_transform_interp_backward(im.data_ptr(), 2, 40, 52, 3, th.data_ptr(), 6, 1, dout.data_ptr(), out[0], out[1],
                                                         buf.data_ptr(), 0, None, None, 0, runtime.stream_ptr()) == 0
    _check("d_img over NaN", buf, r["d_img"], _img_bound(r))


@pytest.mark.parametrize("name,tdim", [("rotation_zoom", 6), ("outside", 8)])
def test_tile_kernel_against_pixel_kernel(name, tdim):
    """A 3-channel image through the tile kernel against its three channels through the pixel kernel: d img within the two atomic-
    order bounds, d theta (the channels' sum) within the two d theta bounds."""
    c = _theta_case(name, 3, tdim)
    im, th, dout, out = c["im"].cuda(), c["theta"].cuda(), c["dout"].cuda(), c["out"]
    parts = [training.st_transform_backward(im[..., k:k + 1].contiguous(), th, dout[..., k:k + 1].contiguous(), out, interp=BC) for k in range(3)]
    d_img = torch.cat([p[0] for p in parts], -1)
    assert bool(((c["d_img"] - d_img).abs().cpu().double() <= 2 * _img_bound(c["r"])).all())
    d_theta = sum(p[1].double() for p in parts).cpu()
    bound = 2 * (R_THETA + 3) * EPS * c["r"]["S_theta"]
    assert bool(((c["d_theta"].cpu().double() - d_theta).abs() <= bound).all())


def test_bilinear_through_the_new_entry_points_is_the_existing_call():
    L, sp = _lib.lib(), runtime.stream_ptr()
    g = torch.Generator().manual_seed(9)
    im = torch.rand(SYM_B, SYM_H, SYM_W, 3, generator=g).cuda()

    def ws(n):
        return torch.zeros(max(int(n), 8), dtype=torch.uint8, device="cuda")

    th = _theta("rotation_zoom", 8).cuda()
    dout = torch.randn(2, 37, 45, 3, generator=g).cuda()
    n = L.vstab_st_transform_backward_workspace_bytes(2, SYM_H, SYM_W, 3, 37, 45)
    a, b, da, db, w = torch.empty(2, 8, device="cuda"), torch.empty(2, 8, device="cuda"), torch.empty_like(im), torch.empty_like(im), ws(n)
    assert L.vstab_st_transform_backward(im.data_ptr(), 2, SYM_H, SYM_W, 3, th.data_ptr(), 8, dout.data_ptr(), 37, 45, da.data_ptr(), 0, a.data_ptr(),
                                         w.data_ptr(), n, sp) == 0
    assert L.vstab_st_transform_interp_backward(im.data_ptr(), 2, SYM_H, SYM_W, 3, th.data_ptr(), 8, 0, dout.data_ptr(), 37, 45, db.data_ptr(), 0,
                                                b.data_ptr(), w.data_ptr(), n, sp) == 0
    assert torch.equal(a, b) and torch.allclose(da, db, rtol=0, atol=1e-4)
    out = (24, 40)
    th = torch.tensor(SYM_THETA['similarity'][out]).cuda()
    dout = torch.randn(2, 40, 24, 3, generator=g).cuda()
    n = L.vstab_st_symmetry_transform_backward_workspace_bytes(2, SYM_H, SYM_W, 3, 24, 40)
    a, b, w = torch.empty(2, 4, device="cuda"), torch.empty(2, 4, device="cuda"), ws(n)
    assert L.vstab_st_symmetry_transform_backward(im.data_ptr(), 2, SYM_H, SYM_W, 3, th.data_ptr(), 2, dout.data_ptr(), 24, 40, None, 0, a.data_ptr(),
                                                  w.data_ptr(), n, sp) == 0
    assert L.vstab_st_symmetry_transform_interp_backward(im.data_ptr(), 2, SYM_H, SYM_W, 3, th.data_ptr(), 2, 0, dout.data_ptr(), 24, 40, None, 0,
                                                         b.data_ptr(), w.data_ptr(), n, sp) == 0
    assert torch.equal(a, b)
    tr = st.ElasticTransformer((40, 56), 4)
    th = (0.15 * torch.randn(2, 32, generator=g)).cuda()
    dout = torch.randn(2, 40, 56, 3, generator=g).cuda()
    n = L.vstab_st_elastic_transform_backward_workspace_bytes(2, SYM_H, SYM_W, 3, 4, 40, 56)
    a, b, w = torch.empty(2, 32, device="cuda"), torch.empty(2, 32, device="cuda"), ws(n)
    assert L.vstab_st_elastic_transform_backward(im.data_ptr(), 2, SYM_H, SYM_W, 3, th.data_ptr(), 4, tr.L_inv.data_ptr(), dout.data_ptr(), 40, 56, None,
                                                 0, a.data_ptr(), w.data_ptr(), n, sp) == 0
    assert L.vstab_st_elastic_transform_interp_backward(im.data_ptr(), 2, SYM_H, SYM_W, 3, th.data_ptr(), 4, tr.L_inv.data_ptr(), 0, dout.data_ptr(), 40,
                                                        56, None, 0, b.data_ptr(), w.data_ptr(), n, sp) == 0
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------- autograd
def _autograd_pairs():
    """(name, transformer built with differentiable=True, theta, the explicit backward) for the six transformers."""
    tps = st.ElasticTransformer((40, 56), 4, interp_method=BC, differentiable=True)
    gen = torch.Generator().manual_seed(4)
    sym_out = (24, 40)
    rows = [("affine", st.AffineTransformer((37, 45), interp_method=BC, differentiable=True), _theta("near_identity", 6),
             lambda im, th, d: training.st_transform_backward(im, th, d, (37, 45), interp=BC)),
            ("projective", st.ProjectiveTransformer((37, 45), interp_method=BC, differentiable=True), _theta("near_identity", 8),
             lambda im, th, d: training.st_transform_backward(im, th, d, (37, 45), interp=BC)),
            ("elastic", tps, 0.15 * torch.randn(2, 32, generator=gen),
             lambda im, th, d: training.st_elastic_transform_backward(im, th, d, (40, 56), 4, tps.L_inv, interp=BC))]
    for kind, k in (("similarity", 2), ("affine_sym", 0), ("projective_sym", 1)):
        cls = {"similarity": st.SimilarityTransformer, "affine_sym": st.AffineSymmetryTransformer, "projective_sym": st.ProjectiveSymmetryTransformer}[kind]
        th = torch.tensor({2: [[0.4, -0.6, 0.3, -0.5], [-0.7, 0.5, -0.2, 0.6]], 0: SYM_THETA['affine'],
                           1: [[3.0, -6.0, 4.0, 5.0, -2.0, -7.0, 8.0, -5.0], [-4.0, 7.0, -9.0, 2.0, 6.0, 3.0, -6.0, 9.0]]}[k])
        rows.append((kind, cls(sym_out, interp_method=BC, differentiable=True), th,
                     lambda im, th, d, k=k: training.st_symmetry_transform_backward(im, th, d, sym_out, k, interp=BC)))
    return rows


@pytest.mark.parametrize("idx", range(6))
def test_autograd_through_transform_is_the_explicit_backward(idx):
    name, tr, theta, explicit = _autograd_pairs()[idx]
    g = torch.Generator().manual_seed(40 + idx)
    im = torch.rand(2, SYM_H, SYM_W, 3, generator=g)
    imc, thc = im.cuda().requires_grad_(True), theta.cuda().requires_grad_(True)
    y = tr.transform(imc, thc)
    assert y.grad_fn is not None, f"{name}: differentiable=True gave no graph"
    dout = torch.randn(y.shape, generator=g).cuda()
    g_im, g_th = torch.autograd.grad(y, (imc, thc), dout)
    e_im, e_th = explicit(im.cuda(), theta.cuda(), dout)
    assert g_th.shape == theta.shape and torch.equal(g_th, e_th)
    assert torch.allclose(g_im, e_im, rtol=0, atol=64 * EPS * float(dout.abs().max()) * 4.5 * 4.5)      # atomic order only
    # without the keyword: today's behaviour, the forward's bits, no graph
    plain = type(tr)(tr.out_size, *([4] if name == "elastic" else []), interp_method=BC).transform(imc, thc)
    assert plain.grad_fn is None and torch.equal(plain, y.detach())
    with torch.no_grad():
        assert tr.transform(imc, thc).grad_fn is None


def test_autograd_frozen_image_or_frozen_theta_skips_that_gradient(monkeypatch):
    c = _theta_case("near_identity", 3, 6)
    calls = []
    real = training.st_transform_backward

    def spy(*a, **k):
        calls.append((k["need_img"], k["need_theta"], k["interp"]))
        res = real(*a, **k)
        calls.append(tuple(t is not None for t in res))
        return res

    monkeypatch.setattr(training, "st_transform_backward", spy)
    tr = st.AffineTransformer(c["out"], interp_method=BC, differentiable=True)
    imc = c["im"].cuda().requires_grad_(True)
    torch.autograd.grad(tr.transform(imc, c["theta"].cuda()), (imc,), c["dout"].cuda())
    assert calls == [(True, False, BC), (True, False)]
    calls.clear()
    thc = c["theta"].cuda().requires_grad_(True)
    (g_th,) = torch.autograd.grad(tr.transform(c["im"].cuda(), thc), (thc,), c["dout"].cuda())
    assert calls == [(False, True, BC), (False, True)] and torch.equal(g_th, c["d_theta"])
    y2 = st.transformer(imc, thc, c["out"], interp_method=BC, differentiable=True)                  # the legacy wrapper passes it through
    assert y2.grad_fn is not None
    assert st.transformer(imc, thc, c["out"], interp_method=BC).grad_fn is None


def test_autograd_through_bicubic_interp_is_the_explicit_backward():
    im, x, y, dout, out, _ = _coords_case(2, 3)
    imc, xc, yc = im.cuda().requires_grad_(True), x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    o = st.bicubic_interp(imc, xc, yc, out, differentiable=True)
    assert o.grad_fn is not None
    g_im, g_x, g_y = torch.autograd.grad(o, (imc, xc, yc), dout.cuda())
    e_im, e_x, e_y = training.st_bicubic_interp_backward(im.cuda(), x.cuda(), y.cuda(), dout.cuda(), out)
    assert torch.equal(g_x, e_x) and torch.equal(g_y, e_y)
    s, leaves = ref.bicubic_interp(im, x, y, out)
    r = ref.backward(s, leaves, dout)
    _check("autograd d_img", g_im, r["d_img"], _img_bound(r))
    plain = st.bicubic_interp(imc, xc, yc, out)
    assert plain.grad_fn is None and torch.equal(plain, o.detach())
    (only_x,) = torch.autograd.grad(st.bicubic_interp(im.cuda(), xc, y.cuda(), out, differentiable=True), (xc,), dout.cuda())
    assert torch.equal(only_x, e_x)


def test_gradient_descent_moves_towards_a_known_affine_shift():
    """theta* = the identity shifted by (0.06, -0.05); from the identity, 12 steps of plain gradient descent (step 0.1) on the MSE
    between the two bicubic transforms of a smooth 48 x 64 x 3 image.  The loss is a smooth bowl in the two translation entries
    around theta*; the assertion (half the starting loss) is a condition, not a measurement."""
    H, W = 48, 64
    im = _smooth_image(H, W).cuda()
    tr = st.AffineTransformer((H, W), interp_method=BC, differentiable=True)
    target = tr.transform(im, torch.tensor([[1.0, 0, 0.06, 0, 1, -0.05]]).cuda())
    theta = torch.tensor([[1.0, 0, 0, 0, 1, 0]], device="cuda", requires_grad=True)
    losses = []
    for _ in range(12):
        loss = ((tr.transform(im, theta) - target) ** 2).mean()
        (g,) = torch.autograd.grad(loss, theta)
        losses.append(float(loss.detach()))
        theta = (theta.detach() - 0.1 * g).requires_grad_(True)
    final = float(((tr.transform(im, theta.detach()) - target) ** 2).mean())
    print(f"loss {losses[0]:.4e} -> {final:.4e}; theta {theta.detach().cpu().tolist()}")
    assert final <= losses[0] / 2


# ------------------------------------------------------------------------------------------------------- argument checks
def test_new_entry_points_reject_bad_arguments():
    L, sp = _lib.lib(), runtime.stream_ptr()
    B, H, W, C_, oh, ow = 1, 104, 117, 3, 6, 7
    im, th = torch.rand(B, H, W, C_, device="cuda"), torch.tensor([[1.0, 0, 0, 0, 1, 0, 0, 0]], device="cuda")
    dout = torch.rand(B, oh, ow, C_, device="cuda")
    x = torch.zeros(B * oh * ow, device="cuda")
    d_img, d_th, d_x = torch.full_like(im, 7.0), torch.full((B, 8), 7.0, device="cuda"), torch.full_like(x, 7.0)
    linv = st.ElasticTransformer((oh, ow), 2).L_inv
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    E_SHAPE, E_NOMEM, E_STATE = -1, -4, -6

    def tb(img=im.data_ptr(), B=B, H=H, tdim=6, ip=1, do=dout.data_ptr(), di=d_img.data_ptr(), dt=d_th.data_ptr(), w=ws.data_ptr(), wb=ws.numel()):
        return L.vstab_st_transform_interp_backward(img, B, H, W, C_, th.data_ptr(), tdim, ip, do, oh, ow, di, 0, dt, w, wb, sp)

    def sb(img=im.data_ptr(), H=H, kind=1, ip=1, di=d_img.data_ptr(), dt=d_th.data_ptr(), w=ws.data_ptr(), wb=ws.numel()):
        return L.vstab_st_symmetry_transform_interp_backward(img, B, H, W, C_, th.data_ptr(), kind, ip, dout.data_ptr(), oh, ow, di, 0, dt, w, wb, sp)

    def eb(img=im.data_ptr(), g=2, ip=1, lv=linv.data_ptr(), di=d_img.data_ptr(), dt=d_th.data_ptr(), w=ws.data_ptr(), wb=ws.numel()):
        return L.vstab_st_elastic_transform_interp_backward(img, B, H, W, C_, th.data_ptr(), g, lv, ip, dout.data_ptr(), oh, ow, di, 0, dt, w, wb, sp)

    def ib(img=im.data_ptr(), B=B, H=H, xx=x.data_ptr(), di=d_img.data_ptr(), dx=d_x.data_ptr()):
        return L.vstab_st_bicubic_interp_backward(img, B, H, W, C_, xx, x.data_ptr(), dout.data_ptr(), oh, ow, di, 0, dx, None, sp)

    for f, name in ((tb, b"st_transform_interp_backward"), (sb, b"st_symmetry_transform_interp_backward"), (eb, b"st_elastic_transform_interp_backward")):
        assert f(H=0) == E_SHAPE if f is not eb else f(g=1) == E_SHAPE
        assert name in L.vstab_last_error(None)
        assert f(ip=2) == E_SHAPE and f(ip=-1) == E_SHAPE
        assert b"unknown interp" in L.vstab_last_error(None) and name in L.vstab_last_error(None)
        assert f(di=None, dt=None) == E_SHAPE and b"both NULL" in L.vstab_last_error(None)
        assert f(wb=0) == E_NOMEM and f(w=None) == E_NOMEM and b"workspace" in L.vstab_last_error(None)
        assert f(img=None) == E_STATE and name in L.vstab_last_error(None)
        assert f(dt=None, w=None, wb=0) == 0 and f(ip=0) == 0 and f() == 0
    assert tb(tdim=7) == E_SHAPE and tb(B=65536) == E_SHAPE and tb(B=0) == E_SHAPE and tb(do=None) == E_STATE
    assert sb(kind=3) == E_SHAPE and sb(H=99) == E_SHAPE and eb(g=17) == E_SHAPE and eb(lv=None) == E_STATE
    assert ib(H=0) == E_SHAPE and ib(B=65536) == E_SHAPE and b"st_bicubic_interp_backward" in L.vstab_last_error(None)
    assert ib(di=None, dx=None) == E_SHAPE and ib(img=None) == E_STATE and ib(xx=None) == E_STATE
    torch.cuda.synchronize()
    d_img.fill_(7.0), d_th.fill_(7.0)
    assert tb(H=0) == E_SHAPE and ib(di=None, dx=None) == E_SHAPE and sb(ip=5) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((d_img == 7.0).all()) and bool((d_th == 7.0).all())                # a refused call writes nothing
    with pytest.raises(ValueError):
        training.st_transform_backward(im, th, dout, (oh, ow), interp='nearest')
