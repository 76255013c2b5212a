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
