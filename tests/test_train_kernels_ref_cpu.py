"""Pins tests/train_kernels_ref.py on the CPU: the Adam reference is torch.optim.Adam where the two agree, its float32 restatement
sets the bound of the GPU test and that bound tells five wrong Adams apart on the GPU test's own inputs; the gather reference is the
oracle's full-resolution head, and its backward is its adjoint."""
import numpy as np
import pytest
import torch

from oracle import vstab_oracle as vo
from tests import train_kernels_ref as ref


# ----------------------------------------------------------------------------- Adam
def test_adam_ref_is_torch_adam_when_eps_is_zero():
    """TF adds eps to sqrt(v) and folds both bias corrections into lr_t; torch adds it to sqrt(v / (1 - b2^t)).  With eps = 0 the two
    are the same function.  The reference rounds its hyper-parameters to float32 as the kernel's arguments are, so torch gets the
    rounded betas, and each step the learning rate whose lr_t is that float32 number."""
    rng = np.random.default_rng(7)
    n, lr = 64, 1e-3
    b1, b2 = float(np.float32(0.9)), float(np.float32(0.999))
    p = torch.tensor(rng.standard_normal(n), dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=0.0)
    w, m, v = p.detach().numpy().copy(), np.zeros(n), np.zeros(n)
    for t in range(1, 6):
        g = rng.standard_normal(n) + 0.1
        step = ref.lr_t(lr, b1, b2, t)
        opt.param_groups[0]["lr"] = float(np.float32(step)) * (1.0 - b1 ** t) / np.sqrt(1.0 - b2 ** t)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        w, m, v = ref.adam_ref(w, g, m, v, step, b1, b2, 0.0, dtype=np.float64)
        state = opt.state[p]
        assert np.abs(m - state["exp_avg"].numpy()).max() <= 1e-12
        assert np.abs(v - state["exp_avg_sq"].numpy()).max() <= 1e-12
        assert np.abs(w - p.detach().numpy()).max() <= 1e-12
    assert float(np.abs(m).min()) > 0.0                          # the state the comparison ran on is not the trivial one


def _run(step_fn, n, b1):
    """Four steps of `step_fn` (same signature as adam_ref with dtype float32), each from its own previous state; the largest error
    in units of every step against one fp64 reference step from that same state."""
    w, m, v, g = ref.adam_case(n, b1)
    state, worst = (w, m, v), np.zeros(3)
    for t in range(1, ref.ADAM_STEPS + 1):
        step = ref.lr_t(ref.ADAM_LR, b1, ref.ADAM_B2, t)
        got = step_fn(state[0], g[t - 1], state[1], state[2], step, b1, ref.ADAM_B2, ref.ADAM_EPS)
        worst = np.maximum(worst, ref.adam_errors(got, state, g[t - 1], step, b1, ref.ADAM_B2, ref.ADAM_EPS))
        state = got
    return worst


def _fp32(w, g, m, v, step, b1, b2, eps):
    return ref.adam_ref(w, g, m, v, step, b1, b2, eps, dtype=np.float32)


def test_adam_fp32_restatement_sets_the_bound():
    worst = np.zeros(3)
    for n, b1 in ref.ADAM_CASES:
        worst = np.maximum(worst, _run(_fp32, n, b1))
    print("float32 restatement, largest error in units (w, m, v):", worst)
    for measured, recorded in zip(worst, ref.ADAM_FP32_UNITS):
        assert recorded - 0.01 < measured <= recorded, (worst, ref.ADAM_FP32_UNITS)
    assert ref.ADAM_BOUND == tuple(4.0 * u for u in ref.ADAM_FP32_UNITS)


def test_adam_case_holds_the_planted_elements():
    w, m, v, g = ref.adam_case(100003, 0.9)
    assert all(a.dtype == np.float32 for a in (w, m, v, g)) and g.shape == (4, 100003)
    free = np.ones(w.size, bool)
    free[list(ref.ADAM_PLANT)] = False
    assert float(np.abs(m[free]).min()) > 0.0 and float(v[free].min()) > 0.0          # the state is nowhere the trivial one
    assert (g[:, 3] == 0).all() and m[3] != 0
    assert (g[:, 17] == 0).all() and m[17] == 0 and v[17] == 0
    assert (np.abs(g[:, 101]) == np.float32(1e4)).all()
    assert (np.abs(g[:, 200]) == np.float32(1e-20)).all() and v[200] == 0 and m[200] != 0
    # (1-b2) g^2 at the last one is a float32 subnormal, not zero: what the 2^-149 in the unit is for
    assert 0.0 < float(np.float32(0.001) * g[0, 200] * g[0, 200]) < 2.0 ** -126
    w1, _, v1 = _fp32(w, g[0], m, v, ref.lr_t(1e-3, 0.9, 0.999, 1), 0.9, 0.999, 1e-8)
    assert w1[3] != w[3] and w1[17] == w[17] and np.isfinite(w1).all()
    step = float(np.float32(ref.lr_t(1e-3, 0.9, 0.999, 1)))
    assert abs((w[200] - w1[200]) / (step * 0.9 * -0.5 / 1e-8) - 1.0) < 1e-5          # sqrt(v) vanishes next to eps: lr_t m / eps


def _mutant(name):
    def f(w, g, m, v, step, b1, b2, eps):
        f32 = np.float32
        step, b1, b2, eps = (f32(x) for x in (step, b1, b2, eps))
        w, g, m, v = (np.asarray(a, dtype=f32) for a in (w, g, m, v))
        one = f32(1.0)
        if name == "betas_swapped":
            b1, b2 = b2, b1
        m1 = (one - b1) * g if name == "b1_m_dropped" else b1 * m + (one - b1) * g
        v1 = b2 * v + g * g if name == "one_minus_b2_dropped" else b2 * v + (one - b2) * g * g
        upd = step * m1 / (np.sqrt(v1 + eps) if name == "eps_inside_sqrt" else np.sqrt(v1) + eps)
        return (w + upd if name == "plus" else w - upd), m1, v1
    return f


@pytest.mark.parametrize("name", ["betas_swapped", "b1_m_dropped", "one_minus_b2_dropped", "eps_inside_sqrt", "plus"])
def test_adam_bound_rejects_wrong_adams(name):
    """Each wrong Adam, stated in float32 like the right one, exceeds the GPU test's bound on the GPU test's inputs: at every size
    that holds all the planted elements.  (eps inside the root differs from eps outside by 1e-8 of the denominator where v is of
    order one -- below float32 -- and shows only where v is tiny: the planted |g| = 1e-20.)"""
    for n, b1 in ref.ADAM_CASES:
        if n <= max(ref.ADAM_PLANT):
            continue
        worst = _run(_mutant(name), n, b1)
        assert any(e > b for e, b in zip(worst, ref.ADAM_BOUND)), (name, n, b1, worst)
    assert all(e <= b for e, b in zip(_run(_mutant("none"), 257, 0.9), ref.ADAM_BOUND))      # the mutant frame itself is a right Adam


# ----------------------------------------------------------------------------- the tap gather and its adjoint
@pytest.mark.parametrize("B,h2,w2,H,W,cs_g", ref.PF2_CASES)
def test_gather_adjoint_identity(B, h2, w2, H, W, cs_g):
    gen = torch.Generator().manual_seed(h2 * 100 + W)
    T = torch.zeros(B, h2, w2, 32, dtype=torch.float64)
    T[..., :18] = torch.randint(-3, 4, (B, h2, w2, 18), generator=gen).double()
    g = torch.randint(-3, 4, (B, H - 2, W - 2, 2), generator=gen).double()
    dT = ref.pf2_taps_backward_ref(g, h2, w2, H, W)
    assert dT.shape == (B, h2, w2, 32) and float(dT[..., 18:].abs().max()) == 0.0
    assert float((ref.pf2_tap_gather(T, H, W) * g).sum()) == float((T * dT).sum())
    # every output pixel's gradient arrives 9 times, less the taps that fall on the zero ring
    iy, ix = vo.nearest_align_corners_index(h2 + 2, H), vo.nearest_align_corners_index(w2 + 2, W)
    inside_y = sum(((iy[d:d + H - 2] >= 1) & (iy[d:d + H - 2] <= h2)).astype(np.int64) for d in range(3))
    inside_x = sum(((ix[d:d + W - 2] >= 1) & (ix[d:d + W - 2] <= w2)).astype(np.int64) for d in range(3))
    ones = ref.pf2_taps_backward_ref(torch.ones(B, H - 2, W - 2, 2), h2, w2, H, W)
    assert float(ones.sum()) == 2.0 * B * float(inside_y.sum()) * float(inside_x.sum())


def test_gather_is_the_oracles_head():
    gen = torch.Generator().manual_seed(11)
    B, h2, w2, Cin, H, W = 2, 5, 6, 7, 18, 23
    concat2 = torch.randn(B, h2, w2, Cin, generator=gen, dtype=torch.float64)
    Wf = torch.randn(3, 3, Cin, 2, generator=gen, dtype=torch.float64)
    want = vo.predict2_fullres(concat2, Wf, torch.zeros(2, dtype=torch.float64), H, W)
    got = ref.pf2_tap_gather(ref.tap_table(concat2, Wf), H, W)
    assert got.shape == want.shape == (B, H - 2, W - 2, 2)
    assert float((got - want).abs().max()) <= 1e-12


def test_column_sum_ref():
    g = torch.arange(2 * 3 * 5, dtype=torch.float32).reshape(2, 3, 5)
    assert ref.column_sum_ref(g, 1, 3).tolist() == [float(sum(range(c, 30, 5))) for c in (1, 2, 3)]


# ----------------------------------------------------------------------------- BatchNorm + lrelu in training mode (tests/bn_train_ref.py)
from functools import lru_cache

from tests import bn_train_ref as bn

F32, F64 = np.float32, np.float64


def _bn_formula(z, beta, eps):
    """The statement of tests/test_gpu_training.py::_bn_ref on a [rows, C] slice, in torch fp64."""
    z = torch.as_tensor(z).double().clone().requires_grad_(True)
    mean = z.mean(dim=0)
    var = ((z - mean) ** 2).mean(dim=0)
    u = (z - mean) / torch.sqrt(var + eps) + torch.as_tensor(beta).double()
    return z, torch.maximum(u, 0.1 * u), mean, var


@pytest.mark.parametrize("rows,cs,c_off,C", [(13, 8, 4, 4), (257, 12, 4, 8), (1000, 72, 4, 68)])
def test_bn_fp64_references_are_autograd_of_the_formula(rows, cs, c_off, C):
    z, beta, mm, mv, dy, eps, decay = bn.bn_case(rows, cs, c_off, C)
    eps = float(F32(eps))
    zt, y, mean, var = _bn_formula(z, beta, eps)
    y.backward(torch.from_numpy(dy).double())
    f = bn.bn_train_forward_ref(z, beta, eps, decay, mm, mv, F64)
    assert np.abs(f["y"] - y.detach().numpy()).max() <= 1e-12
    assert np.abs(f["mean"] - mean.detach().numpy()).max() <= 1e-14 and np.abs(f["var"] - var.detach().numpy()).max() <= 1e-13
    assert np.abs(f["rstd"] - 1 / np.sqrt(var.detach().numpy() + eps)).max() <= 1e-12
    d = float(F32(decay))
    assert np.abs(f["moving_mean"] - (mm.astype(F64) * d + f["mean"] * (1 - d))).max() <= 1e-15
    assert np.abs(f["moving_var"] - (mv.astype(F64) * d + f["var"] * (1 - d))).max() <= 1e-15
    assert (f["y"] > 0).any() and (f["y"] < 0).any()                      # both branches of the gate
    dz, dbeta = bn.bn_train_backward_ref(f["y"], dy, beta, None, F64, z=z, eps=eps)
    assert np.abs(dz - zt.grad.numpy()).max() <= 1e-11 * max(1.0, float(zt.grad.abs().max()))
    gate = np.where(f["y"] > 0, 1.0, 0.1)
    assert np.abs(dbeta - (dy.astype(F64) * gate).sum(axis=0)).max() <= 1e-12 * rows


def test_bn_fp64_backward_is_a_central_finite_difference():
    rng = np.random.default_rng(3)
    rows, C, eps, h = 7, 3, 1e-3, 1e-6
    z, beta, dy = rng.standard_normal((rows, C)) * 2 + 0.5, rng.standard_normal(C), rng.standard_normal((rows, C))

    def loss(zz):
        return float((bn.bn_train_forward_ref(zz, beta, eps, 0.0, None, None, F64)["y"] * dy).sum())

    y = bn.bn_train_forward_ref(z, beta, eps, 0.0, None, None, F64)["y"]
    dz, dbeta = bn.bn_train_backward_ref(y, dy, beta, None, F64, z=z, eps=eps)
    for r in range(rows):
        for c in range(C):
            e = np.zeros_like(z)
            e[r, c] = h
            assert abs((loss(z + e) - loss(z - e)) / (2 * h) - dz[r, c]) <= 1e-7, (r, c)
    for c in range(C):
        e = np.zeros(C)
        e[c] = h
        fd = (float((bn.bn_train_forward_ref(z, beta + e, eps, 0.0, None, None, F64)["y"] * dy).sum()) -
              float((bn.bn_train_forward_ref(z, beta - e, eps, 0.0, None, None, F64)["y"] * dy).sum())) / (2 * h)
        assert abs(fd - dbeta[c]) <= 1e-7


def test_kernel_order_sum_and_chunk_plan():
    assert [bn.chunk_plan(r, C) for r, _, _, C in bn.BN_CASES] == [(1, 1), (1, 13), (1, 16), (1, 17), (1, 127), (1, 255), (2, 128), (2, 129),
                                                                   (7, 143), (16, 129), (17, 129), (76, 169), (768, 129)]
    assert 98311 - 762 * 129 == 13                                         # chunk 762 holds 13 rows, the five after it none
    v = bn.ints((2177, 64), -4, 4, 1).numpy()
    assert np.array_equal(bn.kernel_order_sum(v, F32), v.astype(F64).sum(axis=0).astype(F32))
    assert np.array_equal(bn.kernel_order_sum(v, F64), v.astype(F64).sum(axis=0))
    assert bn.addition_chain(98311, 4) == 33 + 2 + 48 + 16 and bn.addition_chain(1, 4) == 1 + 2 + 1 + 16


def _bn_frame(name):
    """The float32 yardstick restated with one planted mistake; "none" is the yardstick itself.  Forward mistakes act on the forward,
    backward ones ("bwd_...") on the backward, which then runs on the right forward's y."""
    def rows_of(a):
        r = a.shape[0] // 2
        if name.endswith("row_dropped"):
            return np.delete(a, r, axis=0)
        if name.endswith("row_doubled"):
            return np.concatenate([a, a[r:r + 1]])
        return a

    def forward(z, beta, mm, mv, eps, decay):
        fwd = not name.startswith("bwd_")
        rows, z64 = z.shape[0], z.astype(F64)
        zs = rows_of(z64) if fwd else z64
        if zs.shape[0] == 0:
            zs = np.full((1, z.shape[1]), np.nan)
        inv = 1.0 / F64(rows)
        m = bn.kernel_order_sum(zs, F64) * inv
        var = np.maximum(bn.kernel_order_sum(zs * zs, F64) * inv - m * m, 0.0)
        if name == "sample_variance":
            with np.errstate(all="ignore"):
                var = var * (F64(rows) / F64(rows - 1))
        e = F64(F32(eps))
        mean, d, one = m.astype(F32), F32(decay), F32(1)
        rstd = (1.0 / (np.sqrt(var) + e) if name == "eps_outside_root" else 1.0 / np.sqrt(var + e)).astype(F32)
        u = (z - mean) * rstd + beta
        y = np.minimum(u, F32(0.1) * u) if name == "slope_on_wrong_branch" else np.maximum(u, F32(0.1) * u)
        return dict(y=y, mean=mean, rstd=rstd, var=var, moving_mean=mm * d + mean * (one - d), moving_var=mv * d + var.astype(F32) * (one - d))

    def backward(y, dy, beta, rstd):
        rows, pos, tenth = y.shape[0], y > 0, F32(0.1)
        g = np.where(pos, tenth * dy, dy) if name == "bwd_slope_on_wrong_branch" else np.where(pos, dy, tenth * dy)
        xhat = np.where(pos, y, y / tenth) - (F32(0) if name == "bwd_beta_not_subtracted" else beta)
        gs, gxs = (rows_of(g), rows_of(g * xhat)) if name.startswith("bwd_row") else (g, g * xhat)
        if gs.shape[0] == 0:
            gs = gxs = np.full((1, y.shape[1]), np.nan, F32)
        sg, sgx = bn.kernel_order_sum(gs, F32), bn.kernel_order_sum(gxs, F32)
        inv = F32(1) / F32(rows)
        if name == "bwd_gx_term_left_out":
            return rstd * (g - sg * inv), sg
        return rstd * (g - sg * inv - xhat * (sgx * inv)), sg
    return forward, backward


@lru_cache(maxsize=None)
def _bn_yardstick_errors(case, name="none"):
    """Errors in units of every output of the (possibly mutated) float32 statement on one case of BN_CASES."""
    z, beta, mm, mv, dy, eps, decay = bn.bn_case(*case)
    forward, backward = _bn_frame(name)
    with np.errstate(all="ignore"):
        f = forward(z, beta, mm, mv, eps, decay)
        err = bn.bn_forward_errors(f, z, beta, eps, decay, mm, mv)
        right = bn.bn_train_forward_ref(z, beta, eps, decay, mm, mv, F32)
        dz, dbeta = backward(right["y"], dy, beta, right["rstd"])
        err.update(bn.bn_backward_errors(dz, dbeta, right["y"], z, dy, beta, eps))
    if name == "none":
        assert all(np.array_equal(f[k], right[k]) for k in f)
        want = bn.bn_train_backward_ref(right["y"], dy, beta, right["rstd"], F32)
        assert np.array_equal(dz, want[0]) and np.array_equal(dbeta, want[1])
    return err


def test_bn_fp32_yardstick_sets_the_bounds():
    worst = {k: 0.0 for k in bn.BN_FP32_UNITS}
    for case in bn.BN_CASES:
        err = _bn_yardstick_errors(case)
        print("float32 yardstick", case, {k: round(v, 4) for k, v in err.items()})
        worst = {k: max(worst[k], err[k]) for k in worst}
    print("float32 yardstick, largest error in units:", worst)
    for k, recorded in bn.BN_FP32_UNITS.items():
        assert recorded - 0.01 < worst[k] <= recorded, (k, worst, bn.BN_FP32_UNITS)
    assert bn.BN_BOUND == {k: 4.0 * u for k, u in bn.BN_FP32_UNITS.items()}


BN_MISTAKES = ["row_dropped", "row_doubled", "sample_variance", "eps_outside_root", "slope_on_wrong_branch", "bwd_row_dropped", "bwd_row_doubled",
               "bwd_slope_on_wrong_branch", "bwd_beta_not_subtracted", "bwd_gx_term_left_out"]


@pytest.mark.parametrize("name", BN_MISTAKES)
def test_bn_bounds_reject_planted_mistakes(name):
    """Every planted mistake exceeds the GPU test's bound on the GPU test's own inputs, at every shape with more than one row.  (With
    one row xhat is 0, so the sum g xhat term has nothing to contribute; the other mistakes show there too.)  The layer's eps stands
    INSIDE the root, 1 / sqrt(var + eps); the planted mistake moves it outside."""
    for case in bn.BN_CASES:
        err = _bn_yardstick_errors(case, name)
        caught = [k for k, e in err.items() if not e <= bn.BN_BOUND[k]]
        if case[0] > 1 or name != "bwd_gx_term_left_out":
            assert caught, (name, case, err, bn.BN_BOUND)
        side = ("dz", "dbeta") if name.startswith("bwd_") else ("y", "mean", "rstd", "moving_mean", "moving_var")
        assert set(caught) <= set(side)                                   # a mistake shows on its own side only
    assert all(e <= bn.BN_BOUND[k] for k, e in _bn_yardstick_errors(bn.BN_CASES[5]).items())


@pytest.mark.parametrize("rows,C", [(r, C) for r, _, _, C in bn.BN_EXACT_CASES])
def test_bn_exact_cases_are_exact(rows, C):
    """In the exact cases the float32 statement IS the fp64 reference cast to float32, so the GPU test's bit comparison has one right
    answer; a dropped row changes it."""
    z, beta, mm, mv, eps, decay = bn.bn_exact_integer_case(rows, C)
    a, b = (bn.bn_train_forward_ref(z, beta, eps, decay, mm, mv, t) for t in (F32, F64))
    for k in ("mean", "rstd", "moving_mean"):
        assert np.array_equal(a[k], b[k].astype(F32)), k
    assert np.array_equal(a["var"], b["var"])
    z, beta, mm, mv, dy, eps, decay = bn.bn_exact_pm_case(rows, C)
    a, b = (bn.bn_train_forward_ref(z, beta, eps, decay, mm, mv, t) for t in (F32, F64))
    for k in ("y", "mean", "rstd", "moving_mean", "moving_var"):
        assert np.array_equal(a[k], b[k].astype(F32)), k
    assert (a["mean"] == 0).all() and np.array_equal(a["rstd"] * np.abs(z[0]), np.ones(C, F32)) and (a["y"] > 0).all()
    dz32, db32 = bn.bn_train_backward_ref(a["y"], dy, beta, a["rstd"], F32)
    dz64, db64 = bn.bn_train_backward_ref(a["y"], dy, beta, None, F64, z=z, eps=eps)
    assert np.array_equal(dz32, dz64.astype(F32)) and np.array_equal(dz32.astype(F64), dz64) and np.array_equal(db32, db64.astype(F32))
    f_drop = _bn_frame("row_dropped")[0](z, beta, mm, mv, eps, decay)
    assert not np.array_equal(f_drop["mean"], a["mean"]) and not np.array_equal(f_drop["y"], a["y"])


def test_bn_cancellation_bound_holds_for_the_one_pass_statement():
    """The one-pass variance as the kernel states it (double sums in the kernel's order) stays inside the derived bound on the GPU
    test's inputs, and a float32 one-pass variance does not: the bound is not vacuous."""
    for kind in ("near_4096", "plain"):
        z = bn.bn_cancellation_case(kind, 2177, 64)
        want = bn.bn_train_forward_ref(z, np.zeros(64, F32), 1e-5, 0.0, None, None, F64)
        got = bn.bn_train_forward_ref(z, np.zeros(64, F32), 1e-5, 0.0, None, None, F32)
        rel = np.abs(got["rstd"].astype(F64) - want["rstd"]) / want["rstd"]
        bound = bn.rstd_cancellation_bound(z, 1e-5)
        print(kind, "largest |d rstd| / rstd", rel.max(), "bound", bound.min(), "..", bound.max())
        assert (rel <= bound).all()
        m32 = z.mean(axis=0, dtype=F32)
        var32 = np.maximum((z * z).mean(axis=0, dtype=F32) - m32 * m32, 0)
        bad = np.abs(1 / np.sqrt(var32.astype(F64) + 1e-5) - want["rstd"]) / want["rstd"]
        if kind == "near_4096":
            assert (bad > bound).any() and 1e-7 < want["var"].min() and want["var"].max() < 1e-5


def test_lrelu_backward_ref_and_the_exact_tenths():
    """0.1f * dy is exactly dy / 10 for dy = +-10, 20, 30: what lets the zero-y test plant the 0.1 slope into an integer sum."""
    assert [float(F32(0.1) * F32(k)) for k in (10, 20, 30, -10)] == [1.0, 2.0, 3.0, -1.0]
    y, dy = np.array([1, -1, 0.0, -0.0], F32), np.array([3, 3, 3, 3], F32)
    assert np.array_equal(bn.lrelu_backward_ref(y, dy), np.array([3, F32(3) * F32(0.1), F32(3) * F32(0.1), F32(3) * F32(0.1)], F32))


# ----------------------------------------------------------------------------- resampler adjoints
@pytest.mark.parametrize("h,w,oh,ow,C", bn.BILINEAR_CASES + bn.BILINEAR_EXACT_CASES)
def test_bilinear_adjoint_ref_is_autograd_of_the_oracle(h, w, oh, ow, C):
    g, _ = bn.bilinear_case(h, w, oh, ow, C)
    x = torch.randn(2, h, w, C, dtype=torch.float64, generator=torch.Generator().manual_seed(h + ow), requires_grad=True)
    y = vo.resize_bilinear_legacy(x, oh, ow)
    assert np.abs(bn.resize_bilinear_forward_ref(x.detach().numpy(), oh, ow) - y.detach().numpy()).max() <= 1e-13
    if y is x:
        y = x * 1.0
    y.backward(torch.from_numpy(g).double())
    got = bn.resize_bilinear_backward_ref(g, h, w)
    assert np.abs(got - x.grad.numpy()).max() <= 1e-13 * max(1.0, float(x.grad.abs().max()))
    xi, gi = bn.ints((2, h, w, C), -3, 3, h).numpy().astype(F64), bn.ints((2, oh, ow, C), -3, 3, oh).numpy().astype(F64)
    lhs, rhs = float((bn.resize_bilinear_forward_ref(xi, oh, ow) * gi).sum()), float((xi * bn.resize_bilinear_backward_ref(gi, h, w)).sum())
    if (h, w, oh, ow, C) in bn.BILINEAR_EXACT_CASES:
        assert lhs == rhs                                                  # dyadic weights: every product and sum exact
        assert np.array_equal(bn.resize_bilinear_backward_ref(gi, h, w, dtype=F32).astype(F64), bn.resize_bilinear_backward_ref(gi, h, w))
    else:
        assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_bilinear_fp32_restatement_sets_the_bound():
    worst = 0.0
    for case in bn.BILINEAR_CASES:
        h, w = case[:2]
        g, prior = bn.bilinear_case(*case)
        e1 = bn.bilinear_errors(bn.resize_bilinear_backward_ref(g, h, w, dtype=F32), g, h, w)
        e2 = bn.bilinear_errors(bn.resize_bilinear_backward_ref(g, h, w, 2.0, prior, F32), g, h, w, 2.0, prior)
        print("bilinear float32 restatement", case, e1, e2)
        worst = max(worst, e1, e2)
    assert bn.BILINEAR_FP32_UNITS - 0.01 < worst <= bn.BILINEAR_FP32_UNITS, worst
    assert bn.BILINEAR_BOUND == 4.0 * bn.BILINEAR_FP32_UNITS
    # the bound sees one output row missing from a window
    h, w, oh, ow, C = bn.BILINEAR_CASES[0]
    g, _ = bn.bilinear_case(h, w, oh, ow, C)
    short = g.copy()
    short[:, oh - 1] = 0
    assert bn.bilinear_errors(bn.resize_bilinear_backward_ref(short, h, w, dtype=F32), g, h, w) > bn.BILINEAR_BOUND


@pytest.mark.parametrize("h2,w2,H,W", bn.PAD_NEAREST_CASES)
def test_pad_nearest_refs_are_the_oracles_map_and_its_adjoint(h2, w2, H, W):
    src = torch.randn(2, h2, w2, 4, dtype=torch.float64, generator=torch.Generator().manual_seed(h2 + W), requires_grad=True)
    iy, ix = vo.nearest_align_corners_index(h2 + 2, H), vo.nearest_align_corners_index(w2 + 2, W)
    up = torch.nn.functional.pad(src, (0, 0, 1, 1, 1, 1))[:, torch.from_numpy(iy)][:, :, torch.from_numpy(ix)]
    assert np.array_equal(bn.pad_nearest_upsample_ref(src.detach().numpy(), H, W), up.detach().numpy())
    g = bn.ints((2, H, W, 4), -3, 3, H + w2).numpy()
    up.backward(torch.from_numpy(g).double())
    d = bn.pad_nearest_upsample_backward_ref(g, h2, w2)
    assert np.array_equal(d, src.grad.numpy())
    xi = bn.ints((2, h2, w2, 4), -3, 3, W).numpy().astype(F64)
    assert float((bn.pad_nearest_upsample_ref(xi, H, W) * g).sum()) == float((xi * d).sum())
    if H == 1 or W == 1:
        assert not d.any()                                                 # one output row / column: it reads the ring alone
