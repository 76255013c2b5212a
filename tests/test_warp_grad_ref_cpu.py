"""Pins tests/warp_grad_ref.py, the reference of warp.py's gradients, on the CPU: its forward is the oracle's, its autograd gradients
are the central differences of the function it states, and the floor / ceil / zero-row rules give the known answers."""
import math

import pytest
import torch

from oracle import vstab_oracle as vo
from tests import warp_grad_ref as ref

H, W, OUT = 9, 11, (7, 8)
REF = [[3.5, 0.0, 3.9], [0.0, 3.0, 3.3], [0.0, 0.0, 1.0]]                  # canonical grid -> pixels of the 7 x 8 output, off the integers
P_HOMOG = [[0.0313, 0.0521, 0.0417, 0.0611, -0.0337, -0.0453, -0.0229, 0.0383],
           [-0.0719, -0.1103, -0.0631, -0.0907, 0.0541, 0.0877, 0.0353, -0.0467]]
P_AFFINE = [[0.0413, 0.0521, 0.0317, -0.0453, -0.0229, -0.0337], [-0.0631, -0.1103, -0.0719, 0.0877, 0.0353, 0.0541]]


def _img(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("p,kind", [(P_HOMOG, "homography"), (P_AFFINE, "affine")])
def test_forward_is_the_oracles(p, kind):
    im = _img((2, H, W, 3), 1)
    pM = vo.warp_vec2mtrx(torch.tensor(p), kind, 4)
    assert float((ref.vec2mtrx(p, kind, 4)[0].detach() - pM.double()).abs().max()) <= 1e-6          # the oracle's recurrence is fp32
    s, _ = ref.transform(im, pM, OUT, ref=REF)
    want = vo.warp_transform_image(im.double(), vo.warp_compose(REF, pM), OUT[0], OUT[1], dtype=torch.float64, matmul="unfused")
    # the oracle takes xr = xw - floor(xw) in fp32 before the cast, the reference in fp64: one fp32 rounding of a weight at the most
    assert float((s.out.detach() - want).abs().max()) <= 4 * 2.0 ** -24
    plain, _ = ref.transform(im, vo.warp_compose(REF, pM), OUT)
    assert torch.equal(plain.out.detach(), s.out.detach())


def _central(f, leaf, h):
    """central differences of f (-> value, floors) at every element of `leaf`; an element whose +-h evaluations do not share the
    taps of the point itself is left out (NaN).  -> (gradient, share left out)"""
    g = torch.zeros_like(leaf)
    flat = leaf.detach().clone().reshape(-1)
    _, base = f(leaf)
    out = 0
    for i in range(flat.numel()):
        a, b = flat.clone(), flat.clone()
        a[i] += h
        b[i] -= h
        fa, ta = f(a.reshape(leaf.shape))
        fb, tb = f(b.reshape(leaf.shape))
        if all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(base, ta, tb)):
            g.reshape(-1)[i] = (fa - fb) / (2 * h)
        else:
            g.reshape(-1)[i] = float("nan")
            out += 1
    return g, out / flat.numel()


def _close(name, got, want, share, tol=1e-6):
    print(f"{name}: {100 * share:.1f} % of the elements left out (taps change within +-h)")
    assert share <= 0.05, f"{name}: {100 * share:.1f} % left out"
    keep = ~torch.isnan(want)
    assert float((got[keep] - want[keep]).abs().max()) <= tol, name


@pytest.mark.parametrize("kind,approx", [("homography", 1), ("homography", 2), ("homography", 4), ("homography", 8), ("affine", 4)])
def test_gradients_are_central_differences(kind, approx):
    """d M (plain form), d pM (composed form) and d p (through vec2mtrx and the composed warp) on a 7 x 8 grid over a 9 x 11 image."""
    h = 1e-7
    im = _img((2, H, W, 3), 4).double()
    p = torch.tensor(P_HOMOG if kind == "homography" else P_AFFINE, dtype=torch.float64)
    dout = torch.randn(2, OUT[0], OUT[1], 3, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    refm = torch.tensor(REF, dtype=torch.float64)
    pM = ref.vec2mtrx(p, kind, approx, exact=True)[0].detach()
    M = torch.matmul(refm, pM)

    def val(s):
        return float((s.out.detach() * dout).sum()), s.floors

    f_M = lambda m: val(ref.transform(im, m, OUT, exact=True)[0])                                   # noqa: E731
    f_pM = lambda m: val(ref.transform(im, m, OUT, ref=refm, exact=True)[0])                        # noqa: E731
    f_p = lambda q: val(ref.transform(im, ref.vec2mtrx(q, kind, approx, exact=True)[0].detach(), OUT, ref=refm, exact=True)[0])  # noqa: E731
    f_im = lambda i: val(ref.transform(i, M, OUT, exact=True)[0])                                   # noqa: E731

    s, leaves = ref.transform(im, M, OUT, exact=True)
    r = ref.backward(s, leaves, dout)
    _close("d_M", r["d_M"], *_central(f_M, M, h))
    _close("d_img", r["d_img"], *_central(f_im, im, h))
    assert (r["S_M"] >= r["d_M"].abs() - 1e-12).all() and (r["S_img"] >= r["d_img"].abs() - 1e-12).all()
    inside = sum(int(v.sum()) for v in s.inside)
    assert float(r["n_img"][..., 0].sum()) == inside and inside > 2 * OUT[0] * OUT[1]              # every tap inside counts once

    s, leaves = ref.transform(im, pM, OUT, ref=refm, exact=True)
    r = ref.backward(s, leaves, dout)
    _close("d_pM", r["d_M"], *_central(f_pM, pM, h))
    assert (r["S_M"] >= r["d_M"].abs() - 1e-12).all()

    P, p64 = ref.vec2mtrx(p, kind, approx, exact=True)
    s, (_, _) = ref.transform(im, P, OUT, ref=refm, exact=True)
    (d_p,) = torch.autograd.grad(s.out, p64, dout, allow_unused=True)
    d_p = torch.zeros_like(p) if d_p is None else d_p                        # warpApprox = 1: pMtrx = I does not depend on p
    _close("d_p", d_p, *_central(f_p, p, h))
    # the same d p in two steps: d pM from the warp, then vec2mtrx_backward
    two = ref.vec2mtrx_backward(p, r["d_M"], kind, approx, exact=True)
    assert float((two["d_p"] - d_p).abs().max()) <= 1e-12
    assert (two["S_p"] >= two["d_p"].abs() - 1e-12).all()


@pytest.mark.parametrize("kind", ["homography", "affine"])
def test_vec2mtrx_known_answers(kind):
    """warpApprox = 1: pMtrx = I, d p = 0.  warpApprox = 2: pMtrx = I + A, d p is the generator map of d P exactly."""
    p = torch.tensor(P_HOMOG if kind == "homography" else P_AFFINE)
    dP = torch.randn(2, 3, 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    r1 = ref.vec2mtrx_backward(p, dP, kind, 1)
    assert (r1["d_p"] == 0).all() and (r1["S_p"] == 0).all()
    r2 = ref.vec2mtrx_backward(p, dP, kind, 2)
    if kind == "homography":
        want = torch.stack([dP[:, 0, 2], dP[:, 0, 1], dP[:, 0, 0] - dP[:, 1, 1], dP[:, 2, 0], dP[:, 1, 2], dP[:, 1, 0],
                            dP[:, 2, 2] - dP[:, 1, 1], dP[:, 2, 1]], 1)
    else:
        want = dP.reshape(2, 9)[:, :6]
    assert torch.equal(r2["d_p"], want)


def test_integer_translation_and_all_outside_known_answers():
    """9 columns and 5 rows make the grid -1 + i/4, -1 + j/2, exact in fp32, so M = [[4,0,4+tx],[0,2,2+ty],[0,0,1]] hits the pixels
    (i + tx, j + ty) exactly: floor == ceil on both axes, all four taps are that pixel with weights 1, 0, 0, 0, both slopes are 0,
    and d img is dout shifted by (tx, ty) -- each hit pixel counted four times.  An M that sends the whole grid outside the image:
    every gradient is zero."""
    oh, ow, tx, ty = 5, 9, 2, -1
    im = _img((1, oh, ow, 2), 11)
    M = torch.tensor([[[4.0, 0.0, 4.0 + tx], [0.0, 2.0, 2.0 + ty], [0.0, 0.0, 1.0]]])
    s, leaves = ref.transform(im, M, (oh, ow))
    r = ref.backward(s, leaves, torch.ones(1, oh, ow, 2))
    want = torch.zeros(1, oh, ow, 2, dtype=torch.float64)
    want[:, 0:oh + ty, tx:ow] = 1.0                          # output (j, i) adds into source (j + ty, i + tx) where that is inside
    assert torch.equal(r["d_img"], want)
    assert torch.equal(r["n_img"], 4 * want) and torch.equal(r["S_img"], want)
    assert (r["d_M"] == 0).all()
    dout = torch.randn(1, oh, ow, 2, generator=torch.Generator().manual_seed(12), dtype=torch.float64)
    r = ref.backward(*ref.transform(im, M, (oh, ow)), dout)
    assert torch.equal(r["d_img"][:, 0:oh + ty, tx:ow], dout[:, -ty:oh, 0:ow - tx])
    far = torch.tensor([[[0.0, 0.0, -50.0], [0.0, 0.0, -50.0], [0.0, 0.0, 1.0]]])
    r = ref.backward(*ref.transform(im, far, (oh, ow)), dout)
    assert (r["d_img"] == 0).all() and (r["d_M"] == 0).all() and (r["n_img"] == 0).all() and (r["S_M"] == 0).all()
    assert math.isfinite(float(r["S_img"].sum()))
