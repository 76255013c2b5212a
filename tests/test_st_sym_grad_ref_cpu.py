"""Pins tests/st_sym_grad_ref.py, the reference of the symmetric-pad transformers' gradients, on the CPU: its forward is
st_extended_ref.symmetry_transform's, its autograd gradients are the central differences of the fp64 function it states (the
similarity kind at B = 2, so the interleave across samples is differentiated), the affine kind's d theta is exactly zero, and d img
carries every kept pixel's weight once."""
import math

import numpy as np
import pytest
import torch

from tests import st_extended_ref as xref
from tests import st_sym_grad_ref as ref

H, W, C = 104, 117, 2
THETA = {
    'affine': [[0.3, -0.7, 0.2, 0.5, 0.9, -0.4], [-1.1, 0.6, 0.8, -0.2, 0.4, 0.1]],
    'projective': [[3.0, -6.0, 4.0, 5.0, -2.0, -7.0, 8.0, -5.0], [-4.0, 7.0, -9.0, 2.0, 6.0, 3.0, -6.0, 9.0]],
    'similarity': [[0.4, -0.6, 0.3, -0.5], [-0.7, 0.5, -0.2, 0.6]],
}
OUT = (24, 40)


def _smooth(B):
    y, x = torch.meshgrid(torch.linspace(0, 1, H, dtype=torch.float64), torch.linspace(0, 1, W, dtype=torch.float64), indexing='ij')
    ims = []
    for b in range(B):
        ims.append(torch.stack([0.5 + 0.25 * torch.sin(2 * math.pi * (1.0 * x + 0.5 * y) + b) + 0.2 * torch.cos(2 * math.pi * (0.7 * y - 0.4 * x)),
                                0.5 + 0.3 * torch.sin(2 * math.pi * (0.6 * x - 0.9 * y) + 1.0 + 2 * b)], -1))
    return torch.stack(ims)


def _dout(B, seed):
    return torch.randn(B, OUT[1], OUT[0], C, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("kind", ["affine", "projective", "similarity"])
def test_gradients_are_central_differences(kind):
    """exact=True is a plain fp64 function.  The image is a few low-frequency sinusoids, so the bilinear sampler's slope changes
    by O(1e-3) of itself from pixel to pixel and a step of 1e-6 across a pixel boundary costs nothing at the 1e-6 tolerance."""
    B = 2
    im, th, dout = _smooth(B), torch.tensor(THETA[kind], dtype=torch.float64), _dout(B, 3)
    s, leaves = ref.transform(kind, im, th, OUT, exact=True)
    r = ref.backward(s, leaves, dout)
    h = 1e-6

    def f(i, t):
        return float((ref.transform(kind, i, t, OUT, exact=True)[0].out.detach() * dout).sum())

    fd = torch.zeros_like(th)
    for k in range(th.numel()):
        a, b = th.clone().reshape(-1), th.clone().reshape(-1)
        a[k] += h
        b[k] -= h
        fd.reshape(-1)[k] = (f(im, a.reshape(th.shape)) - f(im, b.reshape(th.shape))) / (2 * h)
    scale = max(1.0, float(r["d_theta"].abs().max()))
    assert float((r["d_theta"] - fd).abs().max()) <= 1e-6 * scale, (r["d_theta"], fd)
    if kind == 'affine':
        assert not r["d_theta"].any() and not fd.any() and not r["S_theta"].any()          # the pre-map multiplies by 0
    else:
        assert int((r["d_theta"] != 0).sum()) == th.numel()
    # d img at the pixels with the largest gradient, corners and edges (where the pad folds), and a few others
    flat = r["d_img"].reshape(-1)
    picks = set(torch.topk(flat.abs(), 6).indices.tolist())
    picks |= set(torch.randint(0, flat.numel(), (6,), generator=torch.Generator().manual_seed(4)).tolist())
    for k in picks:
        a, b = im.clone().reshape(-1), im.clone().reshape(-1)
        a[k] += 1e-3                                                            # linear in the image: any step is exact
        b[k] -= 1e-3
        g = (f(a.reshape(im.shape), th) - f(b.reshape(im.shape), th)) / 2e-3
        assert abs(float(flat[k]) - g) <= 1e-9 * max(1.0, abs(g)), (k, float(flat[k]), g)
    assert (r["S_theta"] >= r["d_theta"].abs() * (1 - 1e-12)).all() and (r["S_img"] >= r["d_img"].abs() - 1e-12).all()


@pytest.mark.parametrize("out_size", [(24, 40), (40, 260)])
@pytest.mark.parametrize("kind", ["affine", "projective", "similarity"])
def test_forward_is_the_restatement(kind, out_size):
    """Against st_extended_ref.symmetry_transform (fp32 numpy, explicit np.pad and crop) within the bounds
    tests/test_gpu_st_extended.py allows the kernels: 2e-5 for the fp32 sequence, plus the similarity kind's coordinate term (the
    image is in [0, 1]: a bilinear sample moves by at most 1 per pixel of coordinate); both with and without the fp32 substitution."""
    B = 2
    im, th = _smooth(B).float(), torch.tensor(THETA[kind])
    want = xref.symmetry_transform(kind, im.numpy(), th.numpy(), out_size, 'bilinear')
    if kind == 'affine':
        want = want.reshape(B, out_size[1], out_size[0], C)                    # undo the relabelling: the reference keeps [B, ow, oh, C]
    tol = 2e-5
    if kind == 'similarity':          # that file's similarity bound: cos / sin differ by a few ulp, 2^-20 (|m0| + |m1| + |m2|) per coordinate
        M = np.abs(xref.sym_theta('similarity', th.numpy()).astype(np.float64))
        tol += 2.0 ** -20 * max(M[:, 0:3].sum(1).max(), M[:, 3:6].sum(1).max()) * ((W + 199) / 2 + (H + 199) / 2)
    for exact in (False, True):
        s, _ = ref.transform(kind, im, th, out_size, exact=exact)
        assert tuple(s.out.shape) == want.shape
        assert float(np.abs(s.out.detach().numpy() - want).max()) <= tol
    if out_size == (40, 260):
        assert not s.out[:, :10].any() and not s.out[:, 250:].any()            # the rows the crop-or-pad pads


@pytest.mark.parametrize("out_size", [(24, 40), (40, 260)])
@pytest.mark.parametrize("kind", ["projective", "similarity"])
def test_d_img_sums_to_the_kept_weights(kind, out_size):
    """sum(d img) = sum over the kept pixels and their four taps of w * dout, taps on the zero border excluded: the symmetric pad's
    adjoint moves every contribution and loses none.  n counts the same taps."""
    B = 2
    im, th = _smooth(B).float(), torch.tensor(THETA[kind]) * 4.0                # far enough that some taps reach the zero border
    dout = torch.randn(B, out_size[1], out_size[0], C, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    s, leaves = ref.transform(kind, im, th, out_size)
    r = ref.backward(s, leaves, dout)
    Hp, Wp = H + 200, W + 200
    dfull = ref.to_grid(dout, *out_size).reshape(-1, C)
    kept = ref.to_grid(torch.ones(dout.shape[:3], dtype=torch.float64), *out_size).reshape(-1)
    total, count = 0.0, 0.0
    for w, i in zip(s.wts, s.idx):
        row, col = (i % ((Wp + 2) * (Hp + 2))) // (Wp + 2), i % (Wp + 2)
        inside = ((row >= 1) & (row <= Hp) & (col >= 1) & (col <= Wp)).double()
        total += float(((w * inside).unsqueeze(1) * dfull).sum())
        count += float((inside * kept).sum())
    assert abs(float(r["d_img"].sum()) - total) <= 1e-9 * max(1.0, float(r["S_img"].sum()))
    assert float(r["n_img"][..., 0].sum()) == count and count > 0
    assert float(r["n_pad"][..., 0].sum()) == count
