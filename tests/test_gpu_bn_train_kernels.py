"""BatchNorm in training mode, its backward and the bare leaky-ReLU gate on their own, through the C entry points
(`vstab_bn_lrelu_train_forward`, `vstab_bn_lrelu_train_backward`, `vstab_lrelu_backward`), against tests/bn_train_ref.py.

Exact cases are compared bit for bit; random data within four times the error of the float32 yardstick, in the units of
bn_train_ref's docstring (constants that tests/test_train_kernels_ref_cpu.py re-measures and shows to reject planted mistakes); the
one-pass variance within the bound derived in bn_train_ref.rstd_cancellation_bound.  No tolerance here is a literal.

Channels outside the slice, the two rows behind the last one and the tails of beta / rstd hold NaN; outputs hold NaN beforehand; every
buffer has a tail that is checked afterwards, the scratch beyond vstab_bn_scratch_bytes included; what the kernels must not write
comes back bit-identical."""
import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime
from tests import bn_train_ref as ref

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD, TAIL = 4096, 64
F32, F64 = np.float32, np.float64


def _ptr(t):
    return None if t is None else t.data_ptr()


def _strided(values, cs, c_off):
    """[rows + 2, cs] on the GPU: the slice holds `values`, everything else NaN."""
    rows, C = values.shape
    full = torch.full((rows + 2, cs), NAN)
    full[:rows, c_off:c_off + C] = torch.from_numpy(np.ascontiguousarray(values, F32))
    return full.cuda()


def _only_slice_changed(buf, before, rows, c_off, C):
    a, b = buf.view(torch.int32).clone(), before.view(torch.int32).clone()
    a[:rows, c_off:c_off + C] = 0
    b[:rows, c_off:c_off + C] = 0
    return torch.equal(a, b)


def _vec(values, fill, n=None):
    """values then TAIL elements of `fill`; values None: n NaNs (an output not yet written)."""
    n = len(values) if values is not None else n
    t = torch.full((n + TAIL,), fill)
    t[:n] = NAN if values is None else torch.from_numpy(np.asarray(values, F32))
    return t.cuda()


def _tail_is(t, n, fill):
    tail = t[n:].cpu()
    return bool(torch.isnan(tail).all()) if fill != fill else bool((tail == fill).all())


def _scratch(L, rows, C, fill):
    nbytes = int(L.vstab_bn_scratch_bytes(rows, C))
    assert nbytes > 0
    return torch.full((nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda"), nbytes


def _forward(L, z, beta, mm, mv, eps, decay, cs, c_off, fill=0xA5):
    """One guarded forward call on z [rows, C]: the outputs as numpy arrays and the in-place buffer (for the backward)."""
    rows, C = z.shape
    zy = _strided(z, cs, c_off)
    before = zy.clone()
    b, smean, srstd = _vec(beta, NAN), _vec(None, 7.0, C), _vec(None, 7.0, C)
    mmd, mvd = (None if m is None else _vec(m, 5.0) for m in (mm, mv))
    scratch, nbytes = _scratch(L, rows, C, fill)
    assert L.vstab_bn_lrelu_train_forward(zy.data_ptr(), rows, cs, c_off, C, b.data_ptr(), _ptr(mmd), _ptr(mvd), decay, eps, smean.data_ptr(),
                                          srstd.data_ptr(), scratch.data_ptr(), nbytes, runtime.stream_ptr()) == 0, L.vstab_last_error(None)
    torch.cuda.synchronize()
    assert _only_slice_changed(zy, before, rows, c_off, C)                 # out-of-slice channels and the rows behind: bit-identical
    assert _tail_is(smean, C, 7.0) and _tail_is(srstd, C, 7.0) and _tail_is(b, C, NAN)
    assert all(m is None or _tail_is(m, C, 5.0) for m in (mmd, mvd))
    assert bool((scratch[nbytes:] == fill).all())                          # nothing beyond the scratch size the library asked for
    out = dict(y=zy[:rows, c_off:c_off + C].cpu().numpy(), mean=smean[:C].cpu().numpy(), rstd=srstd[:C].cpu().numpy(),
               moving_mean=None if mmd is None else mmd[:C].cpu().numpy(), moving_var=None if mvd is None else mvd[:C].cpu().numpy())
    assert all(v is None or np.isfinite(v).all() for v in out.values())
    return out, zy


def _backward(L, ybuf, cs_y, cy_off, dy, cs_g, cg_off, beta, rstd, prior=None, dbeta=True, fill=0xA5):
    """One guarded backward call: ybuf a [rows + 2, cs_y] GPU buffer, dy [rows, C] values.  Returns (dz, dbeta) as numpy arrays."""
    rows, C = dy.shape
    dyb = _strided(dy, cs_g, cg_off)
    before, ybefore = dyb.clone(), ybuf.clone()
    b, r = _vec(beta, NAN), _vec(rstd, NAN)
    db = _vec(prior, 7.0, C) if dbeta else None
    scratch, nbytes = _scratch(L, rows, C, fill)
    assert L.vstab_bn_lrelu_train_backward(ybuf.data_ptr(), cs_y, cy_off, dyb.data_ptr(), cs_g, cg_off, C, rows, b.data_ptr(), r.data_ptr(),
                                           _ptr(db), 0 if prior is None else 1, scratch.data_ptr(), nbytes,
                                           runtime.stream_ptr()) == 0, L.vstab_last_error(None)
    torch.cuda.synchronize()
    assert torch.equal(ybuf.view(torch.int32), ybefore.view(torch.int32))  # y is read only
    assert _only_slice_changed(dyb, before, rows, cg_off, C)
    assert _tail_is(b, C, NAN) and _tail_is(r, C, NAN) and (db is None or _tail_is(db, C, 7.0))
    assert bool((scratch[nbytes:] == fill).all())
    dz = dyb[:rows, cg_off:cg_off + C].cpu().numpy()
    assert np.isfinite(dz).all()
    return dz, None if db is None else db[:C].cpu().numpy()


def _same_bits(a, b):
    return all((a[k] is None and b[k] is None) or np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in a)


# ----------------------------------------------------------------------------- random data within the yardstick's bound
@pytest.mark.parametrize("rows,cs,c_off,C", ref.BN_CASES)
def test_bn_forward_then_backward_within_four_yardsticks(rows, cs, c_off, C):
    """Forward, then the backward on the forward's own output, every output against the fp64 reference (two-pass statistics, the
    derivative from the true z) in units; eps and decay vary by case.  The smaller shapes run each call twice with the scratch
    refilled by another byte pattern in between: the sums have a fixed order and depend on nothing left in the scratch."""
    L = _lib.lib()
    z, beta, mm, mv, dy, eps, decay = ref.bn_case(rows, cs, c_off, C)
    got, zy = _forward(L, z, beta, mm, mv, eps, decay, cs, c_off)
    err = ref.bn_forward_errors(got, z, beta, eps, decay, mm, mv)
    dz, dbeta = _backward(L, zy, cs, c_off, dy, cs, c_off, beta, got["rstd"])
    err.update(ref.bn_backward_errors(dz, dbeta, got["y"], z, dy, beta, eps))
    print(f"bn {(rows, cs, c_off, C)} eps={eps} decay={decay}: error in units {({k: round(v, 3) for k, v in err.items()})}, bound {ref.BN_BOUND}")
    assert all(err[k] <= ref.BN_BOUND[k] for k in err), (err, ref.BN_BOUND)
    assert (got["y"] > 0).any() and (rows == 1 or (got["y"] < 0).any())
    if rows == 1:                                                          # variance 0: rstd = 1 / sqrt(eps), y = lrelu(beta)
        assert np.array_equal(got["rstd"], np.full(C, 1.0 / np.sqrt(F64(F32(eps)))).astype(F32))
        assert np.array_equal(got["y"][0], np.maximum(beta, F32(0.1) * beta)) and np.array_equal(got["mean"], z[0])
    if rows * C <= 1000000:
        again, zy2 = _forward(L, z, beta, mm, mv, eps, decay, cs, c_off, fill=0x5A)
        assert _same_bits(got, again)
        dz2, dbeta2 = _backward(L, zy2, cs, c_off, dy, cs, c_off, beta, again["rstd"], fill=0x5A)
        assert np.array_equal(dz.view(np.int32), dz2.view(np.int32)) and np.array_equal(dbeta.view(np.int32), dbeta2.view(np.int32))


# ----------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("rows,cs,c_off,C", ref.BN_EXACT_CASES)
def test_bn_exact_statistics_on_integers(rows, cs, c_off, C):
    """Integer z in [-4, 4], a power-of-two row count: both double sums are exact in any order, so mean, rstd and moving_mean must be
    the fp64 reference cast to float32 and everything the float32 restatement bit for bit.  A dropped, doubled or misplaced row
    changes the mean and shows."""
    L = _lib.lib()
    z, beta, mm, mv, eps, decay = ref.bn_exact_integer_case(rows, C)
    got, _ = _forward(L, z, beta, mm, mv, eps, decay, cs, c_off)
    want64, want32 = (ref.bn_train_forward_ref(z, beta, eps, decay, mm, mv, t) for t in (F64, F32))
    for k in ("mean", "rstd", "moving_mean"):
        assert np.array_equal(got[k], want64[k].astype(F32)), k
    for k in ("y", "mean", "rstd", "moving_mean", "moving_var"):
        assert np.array_equal(got[k], want32[k]), k
    # arguments the training step never passes, on the same exact data: no moving statistics, one of them, decay 0 and 1
    for use_mm, use_mv, d in ((False, False, 0.75), (True, False, 0.75), (False, True, 0.75), (True, True, 0.0), (True, True, 1.0)):
        a, b = mm if use_mm else None, mv if use_mv else None
        g, _ = _forward(L, z, beta, a, b, eps, d, cs, c_off)
        w = ref.bn_train_forward_ref(z, beta, eps, d, a, b, F32)
        assert all((g[k] is None and w[k] is None) or np.array_equal(g[k], w[k]) for k in g), (use_mm, use_mv, d)
        if d == 0.0:
            assert np.array_equal(g["moving_mean"], g["mean"]) and np.array_equal(g["moving_var"], want64["var"].astype(F32))
        if d == 1.0:
            assert np.array_equal(g["moving_mean"], mm) and np.array_equal(g["moving_var"], mv)


@pytest.mark.parametrize("rows,cs,c_off,C", ref.BN_EXACT_CASES)
def test_bn_exact_forward_and_backward_on_plus_minus_a(rows, cs, c_off, C):
    """Half of each channel +a, half -a, eps = 0: mean 0, rstd = 1 / a, xhat = +-1, integer beta with every u > 0, integer dy.  Every
    output of the forward and dz, dbeta of the backward equal the fp64 reference cast to float32; accumulating onto an integer prior
    is exact too."""
    L = _lib.lib()
    z, beta, mm, mv, dy, eps, decay = ref.bn_exact_pm_case(rows, C)
    got, zy = _forward(L, z, beta, mm, mv, eps, decay, cs, c_off)
    want = ref.bn_train_forward_ref(z, beta, eps, decay, mm, mv, F64)
    for k in ("y", "mean", "rstd", "moving_mean", "moving_var"):
        assert np.array_equal(got[k], want[k].astype(F32)), k
    want_dz, want_db = ref.bn_train_backward_ref(want["y"], dy, beta, None, F64, z=z, eps=eps)
    assert float(np.abs(want_db).max()) < 2 ** 24
    dz, dbeta = _backward(L, zy, cs, c_off, dy, cs, c_off, beta, got["rstd"])
    assert torch.equal(torch.from_numpy(dz), torch.from_numpy(want_dz).float()) and want_dz.any()
    assert torch.equal(torch.from_numpy(dbeta), torch.from_numpy(want_db).float())
    prior = ref.ints((C,), -1000, 1000, C).numpy()
    dz2, dbeta2 = _backward(L, zy, cs, c_off, dy, cs, c_off, beta, got["rstd"], prior=prior)
    assert np.array_equal(dz2, dz) and torch.equal(torch.from_numpy(dbeta2), torch.from_numpy(want_db + prior).float())
    dz3, none = _backward(L, zy, cs, c_off, dy, cs, c_off, beta, got["rstd"], dbeta=False)      # dbeta == NULL
    assert none is None and np.array_equal(dz3, dz)


# ----------------------------------------------------------------------------- the one-pass variance
@pytest.mark.parametrize("kind", ["near_4096", "plain"])
@pytest.mark.parametrize("rows,cs,c_off,C", [(2177, 64, 0, 64), (98311, 8, 4, 4)])
def test_bn_one_pass_variance_against_two_passes(kind, rows, cs, c_off, C):
    """The kernel takes var = E[z^2] - mean^2 from one pass in double.  With a mean of 4096 and a spread of a few float32 ulps var is
    comparable to eps = 1e-5 and thirteen digits cancel.  The reference is the fp64 two-pass variance; the bound on |d rstd| / rstd
    is derived from the kernel's addition chain in bn_train_ref.rstd_cancellation_bound, not chosen."""
    L = _lib.lib()
    z = ref.bn_cancellation_case(kind, rows, C)
    beta = np.zeros(C, F32)
    got, _ = _forward(L, z, beta, None, None, 1e-5, 0.9, cs, c_off)
    want = ref.bn_train_forward_ref(z, beta, 1e-5, 0.9, None, None, F64)
    rel = np.abs(got["rstd"].astype(F64) - want["rstd"]) / want["rstd"]
    bound = ref.rstd_cancellation_bound(z, 1e-5)
    print(f"bn one-pass variance {kind} rows={rows}: var {want['var'].min():.3e} .. {want['var'].max():.3e}, largest |d rstd| / rstd "
          f"{rel.max():.3e}, bound {bound.min():.3e} .. {bound.max():.3e}, largest share of the bound {(rel / bound).max():.3f}")
    assert (rel <= bound).all(), (rel.max(), bound)


# ----------------------------------------------------------------------------- layouts and values the training step never passes
def _hand_made_y(rows, C, seed):
    """y = beta + k with integer beta >= 3 and k in [-2, 2] (so y > 0 and xhat = k), integer dy in [-3, 3]; elements 5, 77 of every
    channel hold y = +0.0 and -0.0 with dy a multiple of 10, where 0.1f * dy is exactly dy / 10."""
    rng = np.random.default_rng(seed)
    beta = rng.integers(3, 7, C).astype(F32)
    y = (beta + rng.integers(-2, 3, (rows, C))).astype(F32)
    dy = rng.integers(-3, 4, (rows, C)).astype(F32)
    y[5], y[77] = 0.0, -0.0
    dy[5], dy[77] = 10.0 * rng.integers(1, 4, C), -10.0 * rng.integers(1, 4, C)
    rstd = (2.0 ** (np.arange(C) % 3 - 1)).astype(F32)
    return y, dy, beta, rstd


def test_bn_backward_on_unequal_layouts_and_zero_y_exact():
    """cy_off = 8, cg_off = 4, cs_y = 24, cs_g = 16, C = 6: two different layouts and a channel count that is no multiple of 4, which
    the backward accepts.  At y == 0, of either sign, the kernel's rule is the negative branch: slope 0.1 and xhat = 0 / 0.1 - beta =
    -beta (the forward gives y == 0 only for u == 0, where both branches agree on y but not on the slope; TensorFlow's maximum-based
    lrelu passes the whole gradient to one of its two arguments there, so neither choice is the reference's).  Pinned here.  All
    sums are integers and the row count a power of two, so dz and dbeta have one right answer."""
    L = _lib.lib()
    rows, C, cs_y, cy_off, cs_g, cg_off = 256, 6, 24, 8, 16, 4
    y, dy, beta, rstd = _hand_made_y(rows, C, 1)
    assert np.signbit(y[77]).all() and not np.signbit(y[5]).any()
    g = np.where(y > 0, dy, dy / 10.0).astype(F64)
    xhat = np.where(y > 0, y, 0.0).astype(F64) - beta
    assert np.array_equal(g, np.rint(g)) and np.array_equal(xhat[5], -beta.astype(F64))
    want_db = g.sum(axis=0)
    want_dz = rstd * (g - want_db / rows - xhat * ((g * xhat).sum(axis=0) / rows))
    assert float(np.abs(g * xhat).sum(axis=0).max()) < 2 ** 24
    y32 = ref.bn_train_backward_ref(y, dy, beta, rstd, F32)
    assert np.array_equal(y32[0], want_dz.astype(F32)) and np.array_equal(y32[1], want_db.astype(F32))
    ybuf = _strided(y, cs_y, cy_off)
    dz, dbeta = _backward(L, ybuf, cs_y, cy_off, dy, cs_g, cg_off, beta, rstd)
    assert torch.equal(torch.from_numpy(dz), torch.from_numpy(want_dz).float())
    assert torch.equal(torch.from_numpy(dbeta), torch.from_numpy(want_db).float())
    prior = ref.ints((C,), -1000, 1000, 3).numpy()
    dz2, dbeta2 = _backward(L, ybuf, cs_y, cy_off, dy, cs_g, cg_off, beta, rstd, prior=prior, fill=0x5A)
    assert np.array_equal(dz2, dz) and np.array_equal(dbeta2, (want_db + prior).astype(F32))
    dz3, none = _backward(L, ybuf, cs_y, cy_off, dy, cs_g, cg_off, beta, rstd, dbeta=False)
    assert none is None and np.array_equal(dz3, dz)


@pytest.mark.parametrize("rows,cs_y,cy_off,cs_g,cg_off,C", [(256, 24, 8, 16, 4, 6), (1000, 12, 4, 12, 4, 8), (1, 4, 0, 8, 4, 4), (257, 7, 2, 5, 0, 5)])
def test_lrelu_backward_exact(rows, cs_y, cy_off, cs_g, cg_off, C):
    """dy where y > 0, one rounding of dy * 0.1f elsewhere (y == +-0 included); y and the out-of-slice channels untouched."""
    L = _lib.lib()
    rng = np.random.default_rng(rows + C)
    y = rng.standard_normal((rows, C)).astype(F32)
    y[0, 0] = 0.0
    y[rows // 2, C - 1] = -0.0
    dy = rng.integers(-3, 4, (rows, C)).astype(F32)
    dy[0, 0], dy[rows // 2, C - 1] = 3.0, -2.0
    ybuf, dyb = _strided(y, cs_y, cy_off), _strided(dy, cs_g, cg_off)
    ybefore, before = ybuf.clone(), dyb.clone()
    assert L.vstab_lrelu_backward(ybuf.data_ptr(), cs_y, cy_off, dyb.data_ptr(), cs_g, cg_off, C, rows, runtime.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ybuf.view(torch.int32), ybefore.view(torch.int32)) and _only_slice_changed(dyb, before, rows, cg_off, C)
    got = dyb[:rows, cg_off:cg_off + C].cpu().numpy()
    want = ref.lrelu_backward_ref(y, dy)
    assert np.array_equal(got, want) and want[0, 0] == F32(3) * F32(0.1)


# ----------------------------------------------------------------------------- refusals
def _unchanged(*bufs):
    torch.cuda.synchronize()
    return all(bool((b == 7.0).all()) for b in bufs)


def test_bn_forward_refuses_bad_arguments():
    L = _lib.lib()
    rows, cs, c_off, C = 129, 16, 4, 8
    zy, beta, mm, mv, sm, sr = (torch.full(s, 7.0, device="cuda") for s in ((rows, cs), (C + 4,), (C,), (C,), (C,), (C,)))
    nbytes = int(L.vstab_bn_scratch_bytes(rows, C))
    sc = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    assert L.vstab_bn_scratch_bytes(0, C) == 0 and L.vstab_bn_scratch_bytes(rows, 0) == 0
    st = runtime.stream_ptr()

    def call(zy_=zy.data_ptr(), rows_=rows, c_off_=c_off, C_=C, beta_=beta.data_ptr(), sm_=sm.data_ptr(), sr_=sr.data_ptr(), sc_=sc.data_ptr(),
             nbytes_=nbytes):
        return L.vstab_bn_lrelu_train_forward(zy_, rows_, cs, c_off_, C_, beta_, mm.data_ptr(), mv.data_ptr(), 0.9, 1e-5, sm_, sr_, sc_, nbytes_, st)

    refused = [dict(nbytes_=nbytes - 1), dict(c_off_=12), dict(rows_=0), dict(C_=6), dict(beta_=beta.data_ptr() + 4), dict(zy_=None),
               dict(beta_=None), dict(sm_=None), dict(sr_=None), dict(sc_=None)]
    for kw in refused:
        assert call(**kw) < 0, kw
        assert b"bn_lrelu_train_forward" in L.vstab_last_error(None), kw
    assert call(nbytes_=nbytes - 1) < 0 and b"scratch" in L.vstab_last_error(None)
    assert _unchanged(zy, beta, mm, mv, sm, sr)
    assert call() == 0                                                      # and the same call in order is taken
    torch.cuda.synchronize()
    assert not bool((sr == 7.0).any())


def test_bn_backward_and_lrelu_backward_refuse_bad_arguments():
    L = _lib.lib()
    rows, cs_y, cy_off, cs_g, cg_off, C = 129, 24, 8, 16, 4, 6
    y, dy, beta, rstd, db = (torch.full(s, 7.0, device="cuda") for s in ((rows, cs_y), (rows, cs_g), (C,), (C,), (C,)))
    nbytes = int(L.vstab_bn_scratch_bytes(rows, C))
    sc = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    st = runtime.stream_ptr()

    def call(y_=y.data_ptr(), dy_=dy.data_ptr(), cy_off_=cy_off, cg_off_=cg_off, rows_=rows, beta_=beta.data_ptr(), rstd_=rstd.data_ptr(),
             sc_=sc.data_ptr(), nbytes_=nbytes):
        return L.vstab_bn_lrelu_train_backward(y_, cs_y, cy_off_, dy_, cs_g, cg_off_, C, rows_, beta_, rstd_, db.data_ptr(), 0, sc_, nbytes_, st)

    for kw in (dict(nbytes_=nbytes - 1), dict(cy_off_=19), dict(cg_off_=11), dict(rows_=0), dict(y_=None), dict(dy_=None), dict(beta_=None),
               dict(rstd_=None), dict(sc_=None)):
        assert call(**kw) < 0, kw
        assert b"bn_lrelu_train_backward" in L.vstab_last_error(None), kw

    def gate(y_=y.data_ptr(), dy_=dy.data_ptr(), cy_off_=cy_off, cg_off_=cg_off, rows_=rows):
        return L.vstab_lrelu_backward(y_, cs_y, cy_off_, dy_, cs_g, cg_off_, C, rows_, st)

    for kw in (dict(cy_off_=19), dict(cg_off_=11), dict(rows_=0), dict(y_=None), dict(dy_=None)):
        assert gate(**kw) < 0, kw
        assert b"lrelu_backward" in L.vstab_last_error(None) and b"bn_" not in L.vstab_last_error(None), kw
    assert _unchanged(y, dy, beta, rstd, db)
    assert call() == 0 and gate() == 0
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and not bool((db == 7.0).any())
