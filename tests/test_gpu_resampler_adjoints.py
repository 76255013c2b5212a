"""The decoder's two resampler adjoints and axpby on their own, through the C entry points, against tests/bn_train_ref.py:
`vstab_pad_nearest_upsample` and its backward EXACTLY (an indexed copy; integer gradients, so the adjoint is an integer sum below
2^24), `vstab_resize_bilinear_backward` exactly where the weights are dyadic and otherwise within four times the error of its float32
restatement (BILINEAR_BOUND, re-measured by tests/test_train_kernels_ref_cpu.py), `vstab_axpby` against the float32 two-product sum
with no tolerance.  Outputs hold NaN beforehand and every output buffer has a tail that is checked afterwards."""
import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime
from tests import bn_train_ref as ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
TAIL = 256
F32, F64 = np.float32, np.float64


def _out(shape, prior=None):
    """(flat GPU buffer, its view of `shape`): NaN or `prior` in the view, then TAIL sevens."""
    n = int(np.prod(shape))
    buf = torch.full((n + TAIL,), 7.0)
    buf[:n] = NAN if prior is None else torch.from_numpy(np.asarray(prior, F32)).reshape(-1)
    buf = buf.cuda()
    return buf, buf[:n].view(*shape)


def _tail_ok(buf):
    return bool((buf[-TAIL:] == 7.0).all())


# ----------------------------------------------------------------------------- pad(1) + nearest(align_corners) and its adjoint
@pytest.mark.parametrize("C", [4, 12])
@pytest.mark.parametrize("h2,w2,H,W", ref.PAD_NEAREST_CASES)
def test_pad_nearest_upsample_and_backward_exact(h2, w2, H, W, C):
    """The backward finds the output rows of a source row inside yc +- span, both derived from 1 / sy in float32: the shapes cover
    the identity map, downsampling, ratios of ten and more, and H == 1 / W == 1 where sy == 0 and every output reads the zero ring.
    A window one row short anywhere loses gradient, and the exact comparison sees it."""
    L = _lib.lib()
    B, st = 2, runtime.stream_ptr()
    src = ref.ints((B, h2, w2, C), -3, 3, h2 * 100 + W + C)
    obuf, out = _out((B, H, W, C))
    srcd = src.cuda()
    assert L.vstab_pad_nearest_upsample(srcd.data_ptr(), B, h2, w2, C, out.data_ptr(), H, W, st) == 0
    torch.cuda.synchronize()
    fwd = out.cpu().numpy()
    assert np.array_equal(fwd.view(np.int32), ref.pad_nearest_upsample_ref(src.numpy(), H, W).view(np.int32)) and _tail_ok(obuf)
    g = ref.ints((B, H, W, C), -3, 3, H * 100 + w2 + C)
    want = ref.pad_nearest_upsample_backward_ref(g.numpy(), h2, w2)
    assert float(np.abs(want).max()) < 2 ** 24
    gd = g.cuda()
    dbuf, dsrc = _out((B, h2, w2, C))
    assert L.vstab_pad_nearest_upsample_backward(gd.data_ptr(), B, H, W, C, dsrc.data_ptr(), h2, w2, 0, st) == 0
    torch.cuda.synchronize()
    got = dsrc.cpu()
    assert torch.equal(got, torch.from_numpy(want).float()) and _tail_ok(dbuf)
    prior = ref.ints((B, h2, w2, C), -1000, 1000, C + H)
    dbuf, dsrc = _out((B, h2, w2, C), prior.numpy())
    assert L.vstab_pad_nearest_upsample_backward(gd.data_ptr(), B, H, W, C, dsrc.data_ptr(), h2, w2, 1, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(dsrc.cpu(), (torch.from_numpy(want) + prior.double()).float()) and _tail_ok(dbuf)
    # on the GPU's own results: <forward(x), g> == <x, backward(g)>, integers, summed in fp64 on the host
    assert float((fwd.astype(F64) * g.numpy().astype(F64)).sum()) == float((src.numpy().astype(F64) * got.numpy().astype(F64)).sum())


def test_pad_nearest_upsample_refuses_bad_arguments():
    L = _lib.lib()
    st = runtime.stream_ptr()
    src, out = torch.full((1, 3, 4, 4), 7.0, device="cuda"), torch.full((1, 9, 9, 4), 7.0, device="cuda")
    assert L.vstab_pad_nearest_upsample(src.data_ptr(), 1, 3, 4, 6, out.data_ptr(), 9, 9, st) < 0          # C no multiple of 4
    assert L.vstab_pad_nearest_upsample(None, 1, 3, 4, 4, out.data_ptr(), 9, 9, st) < 0
    assert L.vstab_pad_nearest_upsample_backward(out.data_ptr(), 1, 9, 9, 6, src.data_ptr(), 3, 4, 0, st) < 0
    assert L.vstab_pad_nearest_upsample_backward(out.data_ptr(), 1, 9, 9, 4, None, 3, 4, 0, st) < 0
    assert b"pad_nearest_upsample_backward" in L.vstab_last_error(None)
    torch.cuda.synchronize()
    assert bool((src == 7.0).all()) and bool((out == 7.0).all())


# ----------------------------------------------------------------------------- legacy bilinear resize: the adjoint
def _bilinear_backward(L, g, h, w, gain, prior):
    B, oh, ow, C = g.shape
    gd = torch.from_numpy(g).cuda()
    buf, din = _out((B, h, w, C), prior)
    assert L.vstab_resize_bilinear_backward(gd.data_ptr(), B, oh, ow, C, din.data_ptr(), h, w, gain, 0 if prior is None else 1,
                                            runtime.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert _tail_ok(buf)
    return din.cpu().numpy()


@pytest.mark.parametrize("h,w,oh,ow,C", ref.BILINEAR_CASES)
def test_resize_bilinear_backward_within_four_restatements(h, w, oh, ow, C):
    """Up- and downsampling, non-integer ratios, one-pixel sides and a 15x ratio (the window formula's ceil((iy + 1) / ry) + 1): the
    error against the fp64 adjoint (explicit matrices of the oracle's index map), in units of 2^-24 (|prior| + |gain| A^T |g|)."""
    L = _lib.lib()
    g, prior = ref.bilinear_case(h, w, oh, ow, C)
    e1 = ref.bilinear_errors(_bilinear_backward(L, g, h, w, 1.0, None), g, h, w)
    e2 = ref.bilinear_errors(_bilinear_backward(L, g, h, w, 2.0, prior), g, h, w, 2.0, prior)
    print(f"resize_bilinear_backward {(h, w, oh, ow, C)}: error in units {e1:.3f} (gain 1), {e2:.3f} (gain 2, accumulated), "
          f"bound {ref.BILINEAR_BOUND}")
    assert e1 <= ref.BILINEAR_BOUND and e2 <= ref.BILINEAR_BOUND


@pytest.mark.parametrize("h,w,oh,ow,C", ref.BILINEAR_EXACT_CASES)
def test_resize_bilinear_backward_exact_at_integer_ratios(h, w, oh, ow, C):
    """Integer up-ratios give dyadic weights, so integer gradients give exact sums: the fp64 adjoint cast to float32 is the only right
    answer, and with gain 2 accumulated onto an integer prior it is exactly prior + 2 adjoint."""
    L = _lib.lib()
    g = ref.ints((ref.BILINEAR_B, oh, ow, C), -3, 3, oh + C).numpy()
    want = ref.resize_bilinear_backward_ref(g, h, w)
    got = _bilinear_backward(L, g, h, w, 1.0, None)
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want).float()) and want.any()
    prior = ref.ints((ref.BILINEAR_B, h, w, C), -100, 100, h + C).numpy()
    acc = _bilinear_backward(L, g, h, w, 2.0, prior)
    assert torch.equal(torch.from_numpy(acc), torch.from_numpy(prior.astype(F64) + 2.0 * want).float())


# ----------------------------------------------------------------------------- axpby
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_axpby_is_the_float32_two_product_sum(n):
    """out = a * x + b * y: the kernel states it as two products and a sum and the library is built without contraction, so the float32
    statement is the only right answer.  Also in place (out == x), as the optimiser steps of vgg16.py and NLDF.py call it."""
    L = _lib.lib()
    rng = np.random.default_rng(n)
    x, y = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    buf, out = _out((n,))
    assert L.vstab_axpby(xd.data_ptr(), 0.9, yd.data_ptr(), 0.1, out.data_ptr(), n, runtime.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), F32(0.9) * x + F32(0.1) * y) and _tail_ok(buf)
    buf, p = _out((n,), x)
    assert L.vstab_axpby(p.data_ptr(), 1.0, yd.data_ptr(), -1e-3, p.data_ptr(), n, runtime.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(p.cpu().numpy(), F32(1.0) * x + F32(-1e-3) * y) and _tail_ok(buf)


def test_axpby_refuses_bad_arguments():
    L = _lib.lib()
    x, y, out = (torch.full((8,), 7.0, device="cuda") for _ in range(3))
    st = runtime.stream_ptr()
    assert L.vstab_axpby(x.data_ptr(), 1.0, y.data_ptr(), 1.0, out.data_ptr(), 0, st) < 0
    assert b"axpby" in L.vstab_last_error(None)
    assert L.vstab_axpby(None, 1.0, y.data_ptr(), 1.0, out.data_ptr(), 8, st) < 0
    assert L.vstab_axpby(x.data_ptr(), 1.0, None, 1.0, out.data_ptr(), 8, st) < 0
    assert L.vstab_axpby(x.data_ptr(), 1.0, y.data_ptr(), 1.0, None, 8, st) < 0
    torch.cuda.synchronize()
    assert all(bool((a == 7.0).all()) for a in (x, y, out))
