"""The theta regressors' kernels alone (csrc/theta_ops.hip) against tests/theta_nets_ref.py.

Pad: a copy, bit-equal.  Epilogue, alone and with the pool: bit-equal to the float32 restatement -- the library is built with
-ffp-contract=off, so (z - mean) * rstd + beta is the same three roundings as numpy's, rstd is formed in double and rounded once on both
sides, and slope * u and the maximum are exact selections of one rounding.  Dense: the sums run in another order than numpy's, so the
values are held to the rule of the end-to-end tests (four times the float32 restatement's own distance from float64, never asked to be
closer than FLOOR = 2^-22 of the largest magnitude, which also covers tanhf's two units in the last place); the bit-for-bit statements
are about the kernel's own determinism."""
import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import theta_nets, theta_runtime as tr
from tests import theta_nets_ref as ref

pytestmark = pytest.mark.gpu
FLOOR = 2.0 ** -22


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (7, 9)])
@pytest.mark.parametrize("C,cs", [(1, 4), (3, 4), (27, 28), (64, 64)])
@pytest.mark.parametrize("p", [0, 1])
def test_pad_symmetric(p, C, cs, hw):
    x = np.random.default_rng(C * 10 + p).standard_normal((2, *hw, C)).astype(np.float32)
    xd = dev(x)
    y = tr.pad_symmetric(xd, p, cs)
    assert y.shape == (2, hw[0] + 2 * p, hw[1] + 2 * p, cs)
    assert np.array_equal(bits(y), ref.pad_symmetric(x, p, cs).view(np.uint32))
    assert np.array_equal(xd.cpu().numpy(), x)


def _bn_case(shape, C, seed):
    r = np.random.default_rng(seed)
    z = (r.standard_normal((2, *shape, C)) * 2).astype(np.float32)
    beta, mean = (r.standard_normal(C) * 0.3).astype(np.float32), (r.standard_normal(C) * 0.3).astype(np.float32)
    var = r.uniform(0.5, 1.5, C).astype(np.float32)
    return z, beta, mean, var


@pytest.mark.parametrize("twice", [False, True])
@pytest.mark.parametrize("slope", [0.2, 0.1])
@pytest.mark.parametrize("C", [4, 128])
@pytest.mark.parametrize("hw", [(6, 10), (7, 9), (1, 1)])
def test_epilogue_and_epilogue_with_pool(hw, C, slope, twice):
    z, beta, mean, var = _bn_case(hw, C, C + hw[0])
    want = ref.bn_lrelu(z, beta, mean, var, slope, twice)
    assert want.dtype == np.float32
    zd, b, m, v = dev(z), dev(beta), dev(mean), dev(var)
    pooled = tr.bn_lrelu_slope_pool_inference(zd, b, m, v, slope, twice)
    assert np.array_equal(zd.cpu().numpy(), z)                                       # the fused form reads z only
    assert np.array_equal(bits(pooled), ref.maxpool_same(want).view(np.uint32))
    got = tr.bn_lrelu_slope_inference(zd, b, m, v, slope, twice)
    assert got.data_ptr() == zd.data_ptr() and np.array_equal(bits(got), want.view(np.uint32))


def test_epilogue_on_a_channel_slice_leaves_the_rest():
    z, beta, mean, var = _bn_case((3, 5), 8, 1)
    wide = np.random.default_rng(2).standard_normal((2, 3, 5, 16)).astype(np.float32)
    wide[..., 4:12] = z
    got = tr.bn_lrelu_slope_inference(dev(wide), dev(beta), dev(mean), dev(var), 0.2, False, c_off=4, C=8).cpu().numpy()
    want = wide.copy()
    want[..., 4:12] = ref.bn_lrelu(z, beta, mean, var, 0.2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


KN = [(4, 8), (128, 8), (256, 128), (1000, 1000), (1920, 1000), (40960, 256)]
ACTS = ["identity", "lrelu", "tanh", "tanh_affine"]
_dense_cache = {}


def _dense_case(K, N):
    """x [32,K] (row 3 zeros), W, b, scale, shift on host and device, made once per (K, N); W is scaled so that x . W is O(1)"""
    if (K, N) not in _dense_cache:
        r = np.random.default_rng(K + N)
        x = r.standard_normal((32, K)).astype(np.float32)
        x[3] = 0
        W = (r.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32)
        b = (r.standard_normal(N) * 0.5).astype(np.float32)
        scale, shift = r.uniform(0.5, 2, N).astype(np.float32), r.standard_normal(N).astype(np.float32)
        host = dict(x=x, W=W, b=b, scale=scale, shift=shift)
        _dense_cache[(K, N)] = host, {k: dev(v) for k, v in host.items()}, {}
    return _dense_cache[(K, N)]


def _dense_ref(h, refs, B, act, dtype):
    """ref.dense on all the case's rows, computed once per activation and dtype (the affine tail takes the case's own scale / shift)"""
    key = (act, dtype)
    if key not in refs:
        x, W, b = (h[k].astype(dtype) for k in ("x", "W", "b"))
        if act == "tanh_affine":
            refs[key] = np.tanh(ref.dense(x, W, b) / dtype(1000)) * h["scale"].astype(dtype) + h["shift"].astype(dtype)
        else:
            refs[key] = ref.dense(x, W, b, act, 0.2)
    return refs[key][:B]


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("K,N", KN)
@pytest.mark.parametrize("B", [1, 2, 5, 32])
def test_dense(B, K, N, act):
    h, d, refs = _dense_case(K, N)
    kw = dict(act=act, slope=0.2, scale=d["scale"], shift=d["shift"]) if act == "tanh_affine" else dict(act=act, slope=0.2)
    x = d["x"][:B].contiguous()
    y = tr.dense_forward(x, d["W"], d["b"], **kw)
    assert y.shape == (B, N) and np.array_equal(bits(y), bits(tr.dense_forward(x, d["W"], d["b"], **kw)))          # two calls, equal bits
    r64, r32 = _dense_ref(h, refs, B, act, np.float64), _dense_ref(h, refs, B, act, np.float32)
    mag = np.abs(r64).max()
    err, e32 = np.abs(y.cpu().numpy().astype(np.float64) - r64).max() / mag, np.abs(r32.astype(np.float64) - r64).max() / mag
    print(f"dense B={B} K={K} N={N} {act}: err {err:.2e}, float32 restatement {e32:.2e}, ratio {err / max(e32, 1e-300):.2f}")
    assert err <= max(4 * e32, FLOOR)
    if B == 5:
        one = tr.dense_forward(d["x"][:1].contiguous(), d["W"], d["b"], **kw)
        assert np.array_equal(bits(y)[0], bits(one)[0])                              # a row's bits do not depend on the batch
        # the row of zeros gives act(b): exactly where the activation is a selection, within tanhf's error otherwise
        zero = {k: v[3:4] if k == "x" else v for k, v in h.items()}
        want = _dense_ref(zero, {}, 1, act, np.float32)[0]
        if act in ("identity", "lrelu"):
            assert np.array_equal(bits(y)[3], want.view(np.uint32))
        else:
            assert np.abs(y[3].cpu().numpy() - want).max() <= 4 * np.finfo(np.float32).eps * max(1.0, np.abs(want).max())


def test_dense_scalar_columns():
    """N % 4 != 0 takes the one-column-per-lane kernel: N = 7 and 70 (two tiles)"""
    for K, N in [(64, 7), (260, 70)]:
        r = np.random.default_rng(N)
        x, W, b = r.standard_normal((3, K)).astype(np.float32), (r.standard_normal((K, N)) / np.sqrt(K)).astype(np.float32), r.standard_normal(N).astype(np.float32)
        y = tr.dense_forward(dev(x), dev(W), dev(b)).cpu().numpy().astype(np.float64)
        r64 = ref.dense(x.astype(np.float64), W.astype(np.float64), b.astype(np.float64))
        e32 = np.abs(ref.dense(x, W, b).astype(np.float64) - r64).max()
        assert np.abs(y - r64).max() <= max(4 * e32, FLOOR * np.abs(r64).max())


def test_wrappers_refuse():
    x = torch.zeros(2, 6, device="cuda")
    with pytest.raises(ValueError, match="K a multiple of 4"):
        tr.dense_forward(x, torch.zeros(6, 4, device="cuda"), torch.zeros(4, device="cuda"))
    with pytest.raises(ValueError):
        tr.pad_symmetric(torch.zeros(1, 2, 5, 3, device="cuda"), 3)
    assert theta_nets.LRELU_SLOPE == 0.2
