"""The autograd plumbing of the samplers (_autograd.SamplerFn and the per-op adapters in spatial_transformer.py, warp.py and
warp_flow.py), op by op, at the smallest shapes that reach both kernel forms (C = 3: the tile kernels; C = 2: the pixel kernels).

For every non-empty subset of the inputs that require grad, `backward()` through the op gives
  * parameters and coordinates (theta, x, y, z, M, p, flow): torch.equal to the direct training.*_backward call with the same need_*
    flags -- these sums are reproducible;
  * the image or volume: summed by float atomics, so only close to the direct call -- within the bound the op's own backward test
    allows against the float64 reference (imported from that test, fed by that test's reference);
  * None for every input that does not require grad.
No grad_fn under no_grad, when nothing requires grad, or for the bicubic sampler without differentiable=True; a second backward
through the result raises."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import spatial_transformer as st, training, warp, warp_flow
from tests import st3d_ref, st_bicubic_grad_ref as bref, st_grad_ref as gref, st_sym_grad_ref as sref, st_tps_grad_ref as tref
from tests import warp_flow_grad_ref as fref, warp_grad_ref as wref
from tests.test_gpu_st3d_backward import R_VOL
from tests.test_gpu_st_backward import EPS, _check
from tests.test_gpu_st_bicubic_backward import _img_bound as bicubic_img_bound
from tests.test_gpu_st_sym_backward import _bound_img as sym_img_bound
from tests.test_gpu_st_tps_backward import _img_bound as bilinear_img_bound          # (n + 2) eps S: test_gpu_st_backward.py's, written inline there
from tests.test_gpu_warp_backward import _b_img as warp_img_bound
from tests.test_gpu_warp_flow_backward import _b_img as flow_img_bound

pytestmark = pytest.mark.gpu

PLANE = [(1, 8, 9, 3, 6, 7), (2, 8, 9, 2, 5, 6)]          # B, H, W, C, oh, ow
PADDED = [(1, 104, 117, 3, 6, 7)]                         # the symmetric-pad family needs H, W >= 100
VOLUME = [(1, 4, 5, 6, 2, 3, 4, 5)]                       # B, D, H, W, C, od, oh, ow
SYM = {'affine': st.AffineSymmetryTransformer, 'projective': st.ProjectiveSymmetryTransformer, 'similarity': st.SimilarityTransformer}


def _gen(shape):
    return torch.Generator().manual_seed(sum((i + 1) * v for i, v in enumerate(shape)))


def volume_bound(r):
    return (r["n_vol"] + R_VOL) * EPS * r["S_vol"]


# Every builder returns: names / tensors (CPU float32 inputs, the image or volume first when there is one), forward(*cuda tensors),
# direct(*cuda tensors, dout, needs) -> one gradient or None per tensor, dout_shape, and atomic() -> the bound of tensor 0's
# gradient (None: every gradient is reproducible), plain(*cuda tensors) or None: the same op where it must carry no graph.
def interp_op(shape, bicubic):
    B, H, W, C, oh, ow = shape
    g = _gen(shape)
    im, x, y = torch.rand(B, H, W, C, generator=g), torch.rand(B * oh * ow, generator=g) * 2.4 - 1.2, torch.rand(B * oh * ow, generator=g) * 2.4 - 1.2
    dout = torch.randn(B * oh * ow, C, generator=g)
    fwd = (lambda a, b, c: st.bicubic_interp(a, b, c, (oh, ow), differentiable=True)) if bicubic else (lambda a, b, c: st.bilinear_interp(a, b, c, (oh, ow)))
    back = training.st_bicubic_interp_backward if bicubic else training.st_bilinear_interp_backward
    ref, bound = (bref.bicubic_interp, bicubic_img_bound) if bicubic else (gref.bilinear_interp, bilinear_img_bound)

    def atomic():
        s, leaves = ref(im, x, y, (oh, ow))
        return bound((bref if bicubic else gref).backward(s, leaves, dout))
    return SimpleNamespace(names=("im", "x", "y"), tensors=(im, x, y), dout=dout, forward=fwd, atomic=atomic,
                           direct=lambda a, b, c, d, n: back(a, b, c, d, (oh, ow), need_img=n[0], need_x=n[1], need_y=n[2]),
                           plain=(lambda a, b, c: st.bicubic_interp(a, b, c, (oh, ow))) if bicubic else None)


def theta_op(shape, bicubic):
    B, H, W, C, oh, ow = shape
    g = _gen(shape)
    cls, base = (st.AffineTransformer, [1.0, 0, 0, 0, 1, 0]) if C == 3 else (st.ProjectiveTransformer, [1.0, 0, 0, 0, 1, 0, 0, 0])
    im, theta = torch.rand(B, H, W, C, generator=g), torch.tensor(base).repeat(B, 1) + 0.05 * torch.randn(B, len(base), generator=g)
    dout = torch.randn(B, oh, ow, C, generator=g)
    method = 'bicubic' if bicubic else 'bilinear'
    ref, bound = (bref, bicubic_img_bound) if bicubic else (gref, bilinear_img_bound)

    def atomic():
        s, leaves = ref.transform(im, theta, (oh, ow))
        return bound(ref.backward(s, leaves, dout))
    return SimpleNamespace(names=("im", "theta"), tensors=(im, theta), dout=dout, atomic=atomic,
                           forward=cls((oh, ow), interp_method=method, differentiable=True).transform,
                           direct=lambda a, t, d, n: training.st_transform_backward(a, t, d, (oh, ow), need_img=n[0], need_theta=n[1], interp=method),
                           plain=cls((oh, ow), interp_method=method).transform if bicubic else None)


def symmetry_op(shape, bicubic, kind):
    B, H, W, C, oh, ow = shape
    g = _gen(shape + (len(kind),))
    cls, method = SYM[kind], 'bicubic' if bicubic else 'bilinear'
    tr = cls((oh, ow), interp_method=method, differentiable=True)
    im, theta = torch.rand(B, H, W, C, generator=g), 0.1 * torch.randn(B, cls.param_dim, generator=g)
    out_shape = (B, oh, ow, C) if kind == 'affine' else (B, ow, oh, C)          # AffineSymmetryTransformer relabels its [B,ow,oh,C] result
    dout = torch.randn(out_shape, generator=g)

    def atomic():
        M, (xs, ys) = tr.matrix(theta.cuda()), tr.transform_coords(theta.cuda())
        kw = dict(M32=M.cpu(), xs32=xs.cpu(), ys32=ys.cpu())
        if bicubic:
            s, leaves = bref.symmetry_transform(kind, im, theta, (oh, ow), **kw)
            return bicubic_img_bound(bref.backward(s, leaves, dout.reshape(B, ow, oh, C)))
        s, leaves = sref.transform(kind, im, theta, (oh, ow), **kw)
        return sym_img_bound(sref.backward(s, leaves, dout.reshape(B, ow, oh, C)))

    def direct(a, t, d, n):
        d_img, d_theta = training.st_symmetry_transform_backward(a, t, d.reshape(B, ow, oh, C), (oh, ow), sref.KIND[kind], need_img=n[0],
                                                                 need_theta=n[1], interp=method)
        return d_img, d_theta
    return SimpleNamespace(names=("im", "theta"), tensors=(im, theta), dout=dout, atomic=atomic, forward=tr.transform, direct=direct,
                           plain=cls((oh, ow), interp_method=method).transform if bicubic else None)


def elastic_op(shape, bicubic, grid=2):
    B, H, W, C, oh, ow = shape
    g = _gen(shape)
    method = 'bicubic' if bicubic else 'bilinear'
    tr = st.ElasticTransformer((oh, ow), grid, interp_method=method, differentiable=True)
    im, theta = torch.rand(B, H, W, C, generator=g), 0.15 * torch.randn(B, 2 * grid * grid, generator=g)
    dout = torch.randn(B, oh, ow, C, generator=g)

    def atomic():
        xs, ys = tr.transform_coords(theta.cuda())
        if bicubic:
            s, leaves = bref.elastic(im, xs.cpu(), ys.cpu(), grid, (oh, ow))
            return bicubic_img_bound(bref.elastic_backward(s, leaves, dout, grid, tr.L_inv.cpu()))
        s, leaves = tref.elastic(im, xs.cpu(), ys.cpu(), grid, (oh, ow))
        return bilinear_img_bound(tref.backward(s, leaves, dout, grid, tr.L_inv.cpu()))
    return SimpleNamespace(names=("im", "theta"), tensors=(im, theta), dout=dout, atomic=atomic, forward=tr.transform,
                           direct=lambda a, t, d, n: training.st_elastic_transform_backward(a, t, d, (oh, ow), grid, tr.L_inv, need_img=n[0],
                                                                                           need_theta=n[1], interp=method),
                           plain=st.ElasticTransformer((oh, ow), grid, interp_method=method).transform if bicubic else None)


def interp3d_op(shape, edge=1):
    B, D, H, W, C, od, oh, ow = shape
    g, n, out = _gen(shape), B * od * oh * ow, (od, oh, ow)
    vol = torch.rand(B, D, H, W, C, generator=g)
    x, y, z = (torch.rand(n, generator=g) * 2.4 - 1.2 for _ in range(3))
    dout = torch.randn(n, C, generator=g)

    def atomic():
        s, leaves = st3d_ref.grad_bilinear_interp3d(vol, x, y, z, out, edge)
        return volume_bound(st3d_ref.backward(s, leaves, dout))
    return SimpleNamespace(names=("vol", "x", "y", "z"), tensors=(vol, x, y, z), dout=dout, atomic=atomic, plain=None,
                           forward=lambda v, a, b, c: st.bilinear_interp3d(v, a, b, c, out, edge),
                           direct=lambda v, a, b, c, d, nd: training.st3d_bilinear_interp_backward(v, a, b, c, d, out, edge_size=edge, need_vol=nd[0],
                                                                                                  need_x=nd[1], need_y=nd[2], need_z=nd[3]))


def volume_op(shape):
    B, D, H, W, C, od, oh, ow = shape
    g, out = _gen(shape), (od, oh, ow)
    vol = torch.rand(B, D, H, W, C, generator=g)
    theta = torch.tensor([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]).repeat(B, 1) + 0.05 * torch.randn(B, 12, generator=g)
    dout = torch.randn(B, od, oh, ow, C, generator=g)

    def atomic():
        s, leaves = st3d_ref.grad_transform(vol, theta, out)
        return volume_bound(st3d_ref.backward(s, leaves, dout))
    return SimpleNamespace(names=("vol", "theta"), tensors=(vol, theta), dout=dout, atomic=atomic, plain=None,
                           forward=st.AffineVolumeTransformer(out).transform,
                           direct=lambda v, t, d, n: training.st3d_transform_backward(v, t, d, out, need_vol=n[0], need_theta=n[1]))


def vec2mtrx_op(shape, warp_type):
    B = shape[0] + 1
    dim = 8 if warp_type == "homography" else 6
    g = _gen(shape + (dim,))
    config = SimpleNamespace(warpType=warp_type, warpApprox=8)
    return SimpleNamespace(names=("p",), tensors=(0.1 * torch.randn(B, dim, generator=g),), dout=torch.randn(B, 3, 3, generator=g), atomic=None,
                           plain=None, forward=lambda p: warp.vec2mtrx(config, p),
                           direct=lambda p, d, n: (training.vec2mtrx_backward(p, d, warp_type, 8),))


def warp_op(shape, with_ref):
    B, H, W, C, oh, ow = shape
    g = _gen(shape)
    im, dout = torch.rand(B, H, W, C, generator=g), torch.randn(B, oh, ow, C, generator=g)
    pM = torch.eye(3).repeat(B, 1, 1) + 0.05 * torch.randn(B, 3, 3, generator=g)
    refm = torch.tensor([[(W - 1) / 2, 0.0, (W - 1) / 2], [0.0, (H - 1) / 2, (H - 1) / 2], [0.0, 0.0, 1.0]])       # canonical grid -> source pixels
    if with_ref:
        config = SimpleNamespace(refMtrx=refm, height=oh, width=ow)
        mat, fwd, ref_arg = pM, (lambda a, m: warp.transformImage(config, a, m)), refm
    else:
        mat, fwd, ref_arg = torch.matmul(refm, pM), (lambda a, m: warp.warpImage(a, m, oh, ow)), None

    def atomic():
        s, leaves = wref.transform(im, mat, (oh, ow), ref=ref_arg)
        return warp_img_bound(wref.backward(s, leaves, dout))
    return SimpleNamespace(names=("im", "M"), tensors=(im, mat), dout=dout, atomic=atomic, plain=None, forward=fwd,
                           direct=lambda a, m, d, n: training.homography_warp_backward(a, m, d, (oh, ow), need_img=n[0], need_M=n[1],
                                                                                     ref=None if ref_arg is None else ref_arg.cuda()))


def tf_warp_op(shape):
    B, H, W, C, _, _ = shape
    g = _gen(shape)
    img, flow, dout = torch.rand(B, H, W, C, generator=g), 3.0 * torch.randn(B, H, W, 2, generator=g), torch.randn(B, H, W, C, generator=g)

    def atomic():
        s, leaves = fref.warp(img, flow)
        return flow_img_bound(fref.backward(s, leaves, dout))
    return SimpleNamespace(names=("img", "flow"), tensors=(img, flow), dout=dout, atomic=atomic, plain=None,
                           forward=lambda a, f: warp_flow.tf_warp(a, f, H, W),
                           direct=lambda a, f, d, n: training.warp_flow_backward(a, f, d, need_img=n[0], need_flow=n[1]))


OPS = {}
for _s in PLANE:
    _t = "x".join(map(str, _s))
    for _bc in (False, True):
        _m = "bicubic" if _bc else "bilinear"
        OPS[f"{_m}_interp-{_t}"] = (interp_op, _s, _bc)
        OPS[f"theta_transform_{_m}-{_t}"] = (theta_op, _s, _bc)
        OPS[f"elastic_g2_{_m}-{_t}"] = (elastic_op, _s, _bc)
    OPS[f"vec2mtrx_homography-{_t}"] = (vec2mtrx_op, _s, "homography")
    OPS[f"vec2mtrx_affine-{_t}"] = (vec2mtrx_op, _s, "affine")
    OPS[f"warpImage-{_t}"] = (warp_op, _s, False)
    OPS[f"transformImage-{_t}"] = (warp_op, _s, True)
    OPS[f"tf_warp-{_t}"] = (tf_warp_op, _s)
for _s in PADDED:
    for _bc in (False, True):
        for _k in SYM:
            OPS[f"symmetry_{_k}_{'bicubic' if _bc else 'bilinear'}-{'x'.join(map(str, _s))}"] = (symmetry_op, _s, _bc, _k)
for _s in VOLUME:
    OPS[f"bilinear_interp3d-{'x'.join(map(str, _s))}"] = (interp3d_op, _s)
    OPS[f"volume_transform-{'x'.join(map(str, _s))}"] = (volume_op, _s)


def _leaves(op, requires):
    return [t.cuda().requires_grad_(r) for t, r in zip(op.tensors, requires)]


@pytest.mark.parametrize("name", OPS)
def test_backward_is_the_direct_call_for_every_subset_of_inputs(name):
    build, *args = OPS[name]
    op = build(*args)
    dout = op.dout.cuda()
    bound = op.atomic() if op.atomic is not None else None          # the reference runs once per op
    n = len(op.tensors)
    for requires in itertools.product((False, True), repeat=n):
        if not any(requires):
            continue
        leaves = _leaves(op, requires)
        out = op.forward(*leaves)
        assert out.grad_fn is not None and tuple(out.shape) == tuple(dout.shape), (name, requires)
        out.backward(dout)
        direct = op.direct(*(t.detach() for t in leaves), dout, requires)
        assert len(direct) == n
        for i, (leaf, want, req) in enumerate(zip(leaves, direct, requires)):
            tag = f"{name} d_{op.names[i]} {requires}"
            if not req:
                assert leaf.grad is None and want is None, tag
            elif i == 0 and bound is not None:
                assert leaf.grad.shape == leaf.shape, tag
                _check(tag, leaf.grad, want.reshape(leaf.shape).cpu().double(), bound)
            else:
                assert leaf.grad.shape == leaf.shape and torch.equal(leaf.grad, want.reshape(leaf.shape)), tag
        with pytest.raises(RuntimeError):          # once through: the saved tensors are gone
            out.backward(dout)


@pytest.mark.parametrize("name", OPS)
def test_no_graph_where_none_is_wanted(name):
    build, *args = OPS[name]
    op = build(*args)
    n = len(op.tensors)
    assert op.forward(*_leaves(op, (False,) * n)).grad_fn is None
    with torch.no_grad():
        out = op.forward(*_leaves(op, (True,) * n))
    assert out.grad_fn is None and not out.requires_grad
    if op.plain is not None:                       # the bicubic sampler without differentiable=True
        out = op.plain(*_leaves(op, (True,) * n))
        assert out.grad_fn is None and not out.requires_grad
