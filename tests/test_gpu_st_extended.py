"""The rest of spatial_transformer.py's 2-D samplers on the GPU against the numpy restatement in tests/st_extended_ref.py:
bicubic_interp (ST:966-1072), interp_method='bicubic' on the Affine / Projective transformers, the symmetric-pad transformers
(ST:311-371, 454-517, 611-716) and ElasticTransformer (ST:40-224), plus the C ABI's argument checks.

Tolerances.  Where the kernels and the restatement evaluate the same fp32 sequence (bicubic with given coordinates, the
affine / projective pre-maps) the bound is the sampler tests' 2e-5.  Where they do not -- cos / sin (SimilarityTransformer), the
thin-plate spline's sums, ln and fp32 L_inv table (ElasticTransformer) -- the bound is the source-coordinate error times the
image gradient: for an image in [0, 1] a bilinear sample moves by at most 1 per pixel of coordinate along each axis, a bicubic
one by at most LIP_BICUBIC = max_t sum|w_i'(t)| * max_t sum|w_i(t)| (the derivative of one axis' pass times the gain of the
other's); a normalised coordinate error d becomes d * (n-1)/2 pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime, spatial_transformer as st
from tests import st_extended_ref as ref

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24


def _lip_bicubic():
    t = np.linspace(0, 1, 20001)
    w = [((c[0] + c[1] * t) + c[2] * t * t) + c[3] * t ** 3 for c in ref.BICUBIC_COEFFS]
    dw = [c[1] + 2 * c[2] * t + 3 * c[3] * t * t for c in ref.BICUBIC_COEFFS]
    return float(sum(np.abs(d) for d in dw).max() * sum(np.abs(v) for v in w).max())


LIP = {'bilinear': 1.0, 'bicubic': _lip_bicubic()}          # bicubic: 1.5 * 1.0875 ~ 1.63


def maxabs(a, b):
    return float(np.abs(np.asarray(a.cpu() if torch.is_tensor(a) else a, np.float64) - np.asarray(b, np.float64)).max())


def _img(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------------------------- bicubic
@pytest.mark.parametrize("B,C", [(1, 1), (1, 3), (1, 4), (3, 1), (3, 3), (3, 4)])
def test_bicubic_interp_matches_restatement(B, C):
    H, W, oh, ow = 13, 17, 6, 9
    im = _img((B, H, W, C), 10 * B + C)
    g = torch.Generator().manual_seed(C)
    x = torch.rand(B * oh * ow, generator=g) * 2.6 - 1.3
    y = torch.rand(B * oh * ow, generator=g) * 2.6 - 1.3
    special = torch.tensor([-1.0, 1.0, float("nan"), float("inf"), -float("inf"), 0.0, 1.0 + 1e-7, -3.0, 7.5])
    x[:9] = special
    y[:9] = special.flip(0)
    out = st.bicubic_interp(im.cuda(), x.cuda(), y.cuda(), (oh, ow))
    assert out.shape == (B * oh * ow, C)
    want = ref.bicubic_interp(im.numpy(), x.numpy(), y.numpy(), (oh, ow))
    assert np.isfinite(out.cpu().numpy()).all()
    assert maxabs(out, want) <= 2e-5
    nan_x = x.clone()
    nan_x[torch.isnan(nan_x)] = -1.0                                           # NaN reads as -1
    assert torch.equal(st.bicubic_interp(im.cuda(), nan_x.cuda(), y.cuda(), (oh, ow)), out)
    assert torch.equal(st._interpolate(im.cuda(), x.cuda(), y.cuda(), (oh, ow), 'bicubic'), out)


def test_bicubic_three_channel_tile_path_equals_single_channel_path():
    """C = 3 runs on the tile kernel, C = 1 on the one-thread-per-pixel kernel: the same arithmetic, bit for bit."""
    B, H, W, oh, ow = 2, 45, 70, 37, 61                    # ow % 4 != 0 and a partial tile
    im = _img((B, H, W, 3), 5).cuda()
    g = torch.Generator().manual_seed(2)
    x = (torch.rand(B * oh * ow, generator=g) * 2.4 - 1.2).cuda()
    y = (torch.rand(B * oh * ow, generator=g) * 2.4 - 1.2).cuda()
    out3 = st.bicubic_interp(im, x, y, (oh, ow))
    for c in range(3):
        assert torch.equal(st.bicubic_interp(im[..., c:c + 1].contiguous(), x, y, (oh, ow))[:, 0], out3[:, c])
    for oh2, ow2 in ((16, 32), (20, 44)):                  # ow % 4 == 0: the 16-byte row stores
        x2, y2 = x[:B * oh2 * ow2], y[:B * oh2 * ow2]
        o3 = st.bicubic_interp(im, x2, y2, (oh2, ow2))
        for c in range(3):
            assert torch.equal(st.bicubic_interp(im[..., c:c + 1].contiguous(), x2, y2, (oh2, ow2))[:, 0], o3[:, c])


@pytest.mark.parametrize("B,H,W,C,oh,ow", [(2, 19, 23, 3, 19, 23), (1, 32, 48, 1, 20, 30), (3, 16, 16, 4, 33, 17)])
def test_affine_and_projective_transformer_bicubic(B, H, W, C, oh, ow):
    g = torch.Generator().manual_seed(H * W)
    im = torch.rand(B, H, W, C, generator=g)
    th6 = torch.tensor([1., 0, 0, 0, 1, 0]) + 0.3 * (torch.rand(B, 6, generator=g) - 0.5)
    th8 = torch.cat([th6, 0.2 * (torch.rand(B, 2, generator=g) - 0.5)], 1)
    out = st.AffineTransformer((oh, ow), interp_method='bicubic').transform(im.cuda(), th6.cuda())
    assert out.shape == (B, oh, ow, C)
    assert maxabs(out, ref.transform(im.numpy(), th6.numpy(), (oh, ow), 'bicubic')) <= 2e-5
    outp = st.ProjectiveTransformer((oh, ow), interp_method='bicubic').transform(im.cuda(), th8.cuda())
    assert maxabs(outp, ref.transform(im.numpy(), th8.numpy(), (oh, ow), 'bicubic')) <= 2e-5
    # vstab_st_transform_interp with the bilinear sampler is vstab_st_transform
    L, s = _lib.lib(), runtime.stream_ptr()
    for th, dim in ((th6.cuda(), 6), (th8.cuda(), 8)):
        a = torch.empty(B, oh, ow, C, device="cuda")
        b = torch.empty(B, oh, ow, C, device="cuda")
        imc = im.cuda()
        assert L.vstab_st_transform(imc.data_ptr(), B, H, W, C, th.data_ptr(), dim, a.data_ptr(), oh, ow, s) == 0
        assert L.vstab_st_transform_interp(imc.data_ptr(), B, H, W, C, th.data_ptr(), dim, 0, b.data_ptr(), oh, ow, s) == 0
        assert torch.equal(a, b)
    # identity theta at the input size reproduces the image (bicubic interpolates)
    same = st.AffineTransformer((H, W), interp_method='bicubic').transform(im.cuda(), torch.tensor([1., 0, 0, 0, 1, 0]).repeat(B, 1).cuda())
    assert maxabs(same, im) <= 1e-5


def test_cfg2_size_three_channel_bicubic_affine():
    """configs[2]'s frame size: 720 x 1280 x 3, B = 4, a stabiliser's small rotations / zooms."""
    B, H, W = 4, 720, 1280
    im = _img((B, H, W, 3), 720)
    g = torch.Generator().manual_seed(3)
    a = (torch.rand(B, generator=g) - 0.5) * 0.07
    s = 1 + (torch.rand(B, generator=g) - 0.5) * 0.06
    t = (torch.rand(B, 2, generator=g) - 0.5) * 0.06
    th = torch.stack([s * torch.cos(a), -s * torch.sin(a), t[:, 0], s * torch.sin(a), s * torch.cos(a), t[:, 1]], 1)
    out = st.AffineTransformer((H, W), interp_method='bicubic').transform(im.cuda(), th.cuda())
    assert maxabs(out, ref.transform(im.numpy(), th.numpy(), (H, W), 'bicubic')) <= 2e-5


# ---------------------------------------------------------------------------------------------------- symmetric-pad transformers
_SYM = {'affine': (st.AffineSymmetryTransformer, 6), 'projective': (st.ProjectiveSymmetryTransformer, 8),
        'similarity': (st.SimilarityTransformer, 4)}


@pytest.mark.parametrize("method", ["bilinear", "bicubic"])
@pytest.mark.parametrize("kind", ["affine", "projective", "similarity"])
@pytest.mark.parametrize("H,W,C,B", [(100, 100, 3, 1), (137, 211, 3, 3), (137, 211, 1, 2)])
def test_symmetry_transformers(kind, method, H, W, C, B):
    cls, pdim = _SYM[kind]
    im = _img((B, H, W, C), H + W + C)
    theta = (torch.rand(B, pdim, generator=torch.Generator().manual_seed(B + pdim)) - 0.5) * 2
    for out_size in ((64, 64), (48, 80), (40, 260)):       # square; swapped crop; a crop-or-pad that pads 10 rows
        oh, ow = out_size
        out = cls(out_size, interp_method=method).transform(im.cuda(), theta.cuda())
        want = ref.symmetry_transform(kind, im.numpy(), theta.numpy(), out_size, method)
        assert tuple(out.shape) == want.shape == ((B, oh, ow, C) if kind == 'affine' else (B, ow, oh, C))
        if kind != 'similarity':
            tol = 2e-5                                      # the kernels' own fp32 sequence
        else:
            # fp32 cos / sin (a few ulp) vs numpy's: each matrix entry is off by <= 4 ulp, the coordinate by
            # <= 2^-20 (|m0| + |m1| + |m2|) normalised, times (n+200-1)/2 pixels per axis
            M = np.abs(ref.sym_theta('similarity', theta.numpy()).astype(np.float64))
            d = 2.0 ** -20 * max(M[:, 0:3].sum(1).max(), M[:, 3:6].sum(1).max())
            tol = LIP[method] * d * ((W + 199) / 2 + (H + 199) / 2) + 2e-5
        assert maxabs(out, want) <= tol, (out_size, maxabs(out, want), tol)
        if out_size == (40, 260):
            rows = out.reshape(B, ow, oh, C) if kind == 'affine' else out
            assert not rows[:, :10].any() and not rows[:, 250:].any()          # the pad rows are zeros
    if C == 3:                                              # the tile kernel against the one-thread-per-pixel kernel
        o3 = cls((48, 80), interp_method=method).transform(im.cuda(), theta.cuda())
        for c in range(3):
            o1 = cls((48, 80), interp_method=method).transform(im[..., c:c + 1].contiguous().cuda(), theta.cuda())
            assert torch.equal(o1[..., 0], o3[..., c])


def test_symmetry_identity_and_refusals():
    im = _img((1, 120, 150, 3), 1).cuda()
    # the affine pre-map is the identity for any finite theta: the result is the centre crop of an identity AffineTransformer
    # over the explicitly padded image on the (oh+200) x (ow+200) grid, bit for bit
    out = st.AffineSymmetryTransformer((64, 64)).transform(im, torch.randn(1, 6, device="cuda"))
    pad = torch.from_numpy(np.pad(im.cpu().numpy(), ((0, 0), (100, 100), (100, 100), (0, 0)), mode='symmetric')).cuda()
    full = st.AffineTransformer((264, 264)).transform(pad, torch.tensor([[1., 0, 0, 0, 1, 0]], device="cuda"))
    assert torch.equal(out, full[:, 100:164, 100:164])
    bad = torch.tensor([[float("nan"), 0, 0, 0, 0, 0]], device="cuda")      # NaN survives the * 0
    assert torch.isnan(st.AffineSymmetryTransformer((64, 64)).transform(im, bad)).sum() == 0       # NaN coordinates clip
    for cls, pdim in _SYM.values():
        with pytest.raises(ValueError):
            cls((32, 32)).transform(torch.zeros(1, 99, 120, 3, device="cuda"), torch.zeros(1, pdim, device="cuda"))
        with pytest.raises(ValueError):
            cls((32, 32)).transform(torch.zeros(1, 120, 99, 1, device="cuda"), torch.zeros(1, pdim, device="cuda"))


# ---------------------------------------------------------------------------------------------------- thin-plate spline
def _tps_tolerance(theta, g, out_size, H, W, method, linv):
    """|out - restatement| bound per output pixel: the kernel's fp32 coefficient sums (K terms) and per-pixel sums (K+3 terms)
    with fp32 r^2 ln r^2 are within (K+16) 2^-24 (sum |terms|) of the fp64 coordinates, plus 2^-24 |x| for rounding the
    restatement's coordinates to fp32; times (n-1)/2 pixels and the sampler's gradient bound."""
    K = g * g
    xs, ys, Tabs, Tcoef = ref.tps_coords(theta, g, out_size, linv)
    d = (K + 16) * EPS * (Tabs + Tcoef) + EPS * np.abs(np.stack([xs, ys], 1))
    tol = LIP[method] * (d[:, 0] * (W - 1) / 2 + d[:, 1] * (H - 1) / 2) + 2e-5
    return xs, ys, tol.reshape(-1, out_size[0], out_size[1], 1)


@pytest.mark.parametrize("method", ["bilinear", "bicubic"])
@pytest.mark.parametrize("g", [2, 4, 5])
def test_elastic_transformer(g, method):
    B, H, W, oh, ow = 2, 48, 64, 40, 56
    K = g * g
    tr = st.ElasticTransformer((oh, ow), g, interp_method=method)
    assert tr.param_dim == 2 * K and tuple(tr.L_inv.shape) == (K, K + 3)
    linv = tr.L_inv.cpu().numpy()
    for C in (3, 1):
        im = _img((B, H, W, C), g * 10 + C)
        # theta = 0: the identity map, compared with an identity AffineTransformer
        zero = torch.zeros(B, 2 * K)
        out0 = tr.transform(im.cuda(), zero.cuda())
        ident = st.AffineTransformer((oh, ow), interp_method=method).transform(im.cuda(), torch.tensor([[1., 0, 0, 0, 1, 0]] * B).cuda())
        xs, ys, tol = _tps_tolerance(zero.numpy(), g, (oh, ow), H, W, method, linv)
        xt, yt = ref.grid(oh, ow)
        dev = np.maximum(np.abs(xs - xt).max() * (W - 1) / 2, np.abs(ys - yt).max() * (H - 1) / 2)   # fp32 table vs exact identity
        assert (np.abs(out0.cpu().numpy() - ident.cpu().numpy()) <= tol + 2 * LIP[method] * dev).all()
        # random control-point offsets against the restatement
        theta = 0.15 * torch.randn(B, 2 * K, generator=torch.Generator().manual_seed(g))
        out = tr.transform(im.cuda(), theta.cuda())
        assert out.shape == (B, oh, ow, C)
        xs, ys, tol = _tps_tolerance(theta.numpy(), g, (oh, ow), H, W, method, linv)
        want = ref.interpolate(im.numpy(), xs.reshape(-1).astype(np.float32), ys.reshape(-1).astype(np.float32), (oh, ow),
                               method).reshape(B, oh, ow, C)
        err = np.abs(out.cpu().numpy() - want)
        assert (err <= tol).all(), (float(err.max()), float(tol.min()))
        assert torch.equal(tr.transform(im.cuda(), theta.cuda(), forward=False), out)
        if C == 3:
            o3 = out
        else:
            im3 = _img((B, H, W, 3), g * 10 + 3)
            for c in range(3):                               # the tile kernel against the one-thread-per-pixel kernel
                assert torch.equal(tr.transform(im3[..., c:c + 1].contiguous().cuda(), theta.cuda())[..., 0], o3[..., c])


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_extended_entry_points_reject_bad_arguments():
    L = _lib.lib()
    s = runtime.stream_ptr()
    img = torch.zeros(1, 120, 120, 3, device="cuda")
    x = torch.zeros(64, device="cuda")
    out = torch.zeros(1, 300, 300, 3, device="cuda")
    th = torch.zeros(1, 32, device="cuda")
    p, q, o, t = img.data_ptr(), x.data_ptr(), out.data_ptr(), th.data_ptr()
    assert L.vstab_st_bicubic_interp(p, 1, 120, 120, 3, q, q, 8, 8, o, s) == 0
    assert L.vstab_st_bicubic_interp(None, 1, 120, 120, 3, q, q, 8, 8, o, s) == -6
    assert L.vstab_st_bicubic_interp(p, 1, 120, 120, 3, q, None, 8, 8, o, s) == -6
    assert L.vstab_st_bicubic_interp(p, 0, 120, 120, 3, q, q, 8, 8, o, s) == -1
    assert L.vstab_st_bicubic_interp(p, 1, 120, 120, 0, q, q, 8, 8, o, s) == -1
    assert L.vstab_st_bicubic_interp(p, 1, 120, 120, 3, q, q, 0, 8, o, s) == -1
    assert L.vstab_st_bicubic_interp(p, 70000, 1, 1, 3, q, q, 1, 1, o, s) == -1          # B beyond the grid's y extent
    assert b"st_bicubic_interp" in L.vstab_last_error(None)
    assert L.vstab_st_transform_interp(p, 1, 120, 120, 3, t, 6, 1, o, 8, 8, s) == 0
    assert L.vstab_st_transform_interp(p, 1, 120, 120, 3, t, 7, 1, o, 8, 8, s) == -1      # theta_dim
    assert L.vstab_st_transform_interp(p, 1, 120, 120, 3, t, 6, 2, o, 8, 8, s) == -1      # interp
    assert L.vstab_st_transform_interp(p, 1, 120, 120, 3, None, 6, 1, o, 8, 8, s) == -6
    assert L.vstab_st_symmetry_transform(p, 1, 120, 120, 3, t, 2, 0, o, 8, 8, s) == 0
    assert L.vstab_st_symmetry_transform(p, 1, 99, 120, 3, t, 2, 0, o, 8, 8, s) == -1     # H < 100
    assert L.vstab_st_symmetry_transform(p, 1, 120, 99, 3, t, 2, 0, o, 8, 8, s) == -1     # W < 100
    assert L.vstab_st_symmetry_transform(p, 1, 120, 120, 3, t, 3, 0, o, 8, 8, s) == -1    # kind
    assert L.vstab_st_symmetry_transform(p, 1, 120, 120, 3, t, 0, -1, o, 8, 8, s) == -1   # interp
    assert L.vstab_st_symmetry_transform(p, 1, 120, 120, 3, t, 0, 0, o, -5, 8, s) == -1
    assert L.vstab_st_symmetry_transform(p, 1, 120, 120, 3, t, 0, 0, None, 8, 8, s) == -6
    assert b"st_symmetry_transform" in L.vstab_last_error(None)
    linv = torch.zeros(16 * 19, device="cuda")
    lp = linv.data_ptr()
    assert L.vstab_st_elastic_transform(p, 1, 120, 120, 3, t, 4, lp, 0, o, 8, 8, s) == 0
    assert L.vstab_st_elastic_transform(p, 1, 120, 120, 3, t, 1, lp, 0, o, 8, 8, s) == -1  # g = 1
    assert L.vstab_st_elastic_transform(p, 1, 120, 120, 3, t, 17, lp, 0, o, 8, 8, s) == -1
    assert L.vstab_st_elastic_transform(p, 1, 120, 120, 3, t, 4, None, 0, o, 8, 8, s) == -6
    assert L.vstab_st_elastic_transform(p, 1, 120, 120, 3, t, 4, lp, 5, o, 8, 8, s) == -1
    assert L.vstab_st_elastic_transform(p, 1, 120, 0, 3, t, 4, lp, 0, o, 8, 8, s) == -1
    assert b"st_elastic_transform" in L.vstab_last_error(None)
    torch.cuda.synchronize()
    # the Python layer
    with pytest.raises(ValueError):
        st.ElasticTransformer((8, 8), 1)
    with pytest.raises(ValueError):
        st.ElasticTransformer((8, 8), 17)
    with pytest.raises(ValueError):
        st.ElasticTransformer((8, 8), 4).transform(img, torch.zeros(1, 31, device="cuda"))
    with pytest.raises(NotImplementedError):
        st.AffineTransformer((8, 8), interp_method='nearest').transform(img, torch.zeros(1, 6, device="cuda"))
    with pytest.raises(ValueError):
        st.bicubic_interp(img, x[:3], x[:3], (2, 2))
