"""tests/nldf_head_grad_ref.py (the float64 numpy backward of the NLDF head) against torch.autograd in float64: every stage at tiny
shapes, the contrast layer's self-adjointness at the sizes where its rows differ, the whole walk at the head's real 176 .. 11
geometry with few channels, and one central finite difference of a random directional derivative."""
import numpy as np
import pytest
import torch

from tests import nldf_head_grad_ref as ref

F64 = torch.float64
HW = (176, 88, 44, 22, 11)
FEA = 8
POOL_C = (4, 4, 8, 8, 8)
TOL = 1e-10


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


def vjp(fn, inputs, gout):
    return [g.numpy() for g in ref._vjp(fn, [torch.as_tensor(a) for a in inputs], torch.as_tensor(gout))]


@pytest.mark.parametrize("k,pad,hw", [(1, 0, 5), (3, 1, 4), (3, 0, 3), (5, 0, 7), (3, 1, 1)])
def test_conv_stage(k, pad, hw):
    rng = np.random.default_rng(k * 10 + hw)
    x, W, b = rng.standard_normal((2, hw, hw, 3)), rng.standard_normal((k, k, 3, 5)), rng.standard_normal(5)
    ho = hw + 2 * pad - k + 1
    g = rng.standard_normal((2, ho, ho, 5))
    dx, dW, db = vjp(lambda x_, W_, b_: ref.t_conv(x_, W_, b_, pad), (x, W, b), g)
    assert rel(ref.conv_dgrad(g, W, pad, hw), dx) <= TOL
    gW, gb = ref.conv_wgrad(x, g, k, pad)
    assert rel(gW, dW) <= TOL and rel(gb, db) <= TOL


@pytest.mark.parametrize("h", [1, 2, 3, 6])
def test_transposed_conv_stage(h):
    rng = np.random.default_rng(h)
    x, W, b = rng.standard_normal((2, h, h, 3)), rng.standard_normal((5, 5, 4, 3)), rng.standard_normal(4)
    g = rng.standard_normal((2, 2 * h, 2 * h, 4))
    dx, dW, db = vjp(ref.t_deconv, (x, W, b), g)
    gx, gW, gb = ref.deconv_backward(g, x, W)
    assert rel(gx, dx) <= TOL and rel(gW, dW) <= TOL and rel(gb, db) <= TOL


@pytest.mark.parametrize("H", [1, 2, 3, 5])
@pytest.mark.parametrize("W", [1, 2, 3, 5])
def test_contrast_layer_is_self_adjoint(H, W):
    rng = np.random.default_rng(H * 7 + W)
    x, g = rng.standard_normal((2, H, W, 3)), rng.standard_normal((2, H, W, 3))
    # errors relative to the input: on a single pixel the layer is identically zero (x - 9 x / 9)
    assert np.abs(ref.contrast(x) - ref.t_contrast(torch.as_tensor(x)).numpy()).max() <= TOL * np.abs(x).max()
    (dx,) = vjp(ref.t_contrast, (x,), g)
    assert np.abs(ref.contrast(g) - dx).max() <= TOL * np.abs(g).max()      # the adjoint is the layer itself
    assert abs(np.vdot(ref.contrast(x), g) - np.vdot(x, ref.contrast(g))) <= 1e-12 * x.size
    # the 1-D clamped box sum as a matrix is symmetric: row 0 = [2,1,0..], a single row = [3]
    n = H
    S = np.zeros((n, n))
    for i in range(n):
        for d in (-1, 0, 1):
            S[i, min(max(i + d, 0), n - 1)] += 1
    assert np.array_equal(S, S.T) and S[0, 0] == (3 if n == 1 else 2)


def test_contrast_gate_stage():
    rng = np.random.default_rng(4)
    pre = rng.standard_normal((2, 4, 5, 3))
    pre[..., 0] = -np.abs(pre[..., 0])                                      # a channel nothing passes
    gP, gLC = rng.standard_normal(pre.shape), rng.standard_normal(pre.shape)

    def fn(z):
        p = torch.relu(z)
        return torch.cat([p, ref.t_contrast(p)], 3)

    (dz,) = vjp(fn, (pre,), np.concatenate([gP, gLC], 3))
    got = ref.contrast_gate_backward(np.maximum(pre, 0), gP, gLC)
    assert rel(got, dz) <= TOL and not got[..., 0].any()


def test_score_stage():
    rng = np.random.default_rng(5)
    ls, gs = rng.standard_normal((2, 4, 3, 2)), rng.standard_normal((2, 1, 1, 2))
    dscore, dprob = rng.standard_normal((2, 4, 3, 2)), rng.standard_normal((2, 4, 3, 1))

    def fn(l, g):
        s = l + g
        return torch.cat([s, torch.softmax(s, 3)[..., 0:1]], 3)

    dl, dg = vjp(fn, (ls, gs), np.concatenate([dscore, dprob], 3))
    prob = torch.softmax(torch.as_tensor(ls + gs), 3)[..., 0:1].numpy()
    gl, gg = ref.score_backward(dscore, prob, dprob)
    assert rel(gl, dl) <= TOL and rel(gg, dg.reshape(2, 2)) <= TOL
    gl, gg = ref.score_backward(dscore)
    assert np.array_equal(gl, dscore) and rel(gg, dscore.sum((1, 2))) <= TOL


@pytest.fixture(scope="module")
def net():
    rng = np.random.default_rng(11)
    hw = ref.synthetic_weights(FEA, POOL_C)
    pools = [rng.standard_normal((2, h, h, c)) for h, c in zip(HW, POOL_C)]
    grads = {"dscore": rng.standard_normal((2, 176, 176, 2)), "dprob": rng.standard_normal((2, 176, 176, 1)),
             "dlocal_fea": rng.standard_normal((2, 176, 176, 5 * FEA)) * 0.1, "dfea_global": rng.standard_normal((2, 1, 1, FEA))}
    tp = [torch.as_tensor(p).requires_grad_(True) for p in pools]
    tw = {k: torch.as_tensor(v).requires_grad_(True) for k, v in hw.items()}
    a = ref.torch_forward(tp, tw)
    return hw, pools, grads, tp, tw, a


def _acts(a):
    return {k: ([p.detach().numpy() for p in v] if k == "pools" else v.detach().numpy()) for k, v in a.items()}


@pytest.mark.parametrize("extra", [False, True])
def test_walk_against_autograd_at_the_real_geometry(net, extra):
    hw, pools, grads, tp, tw, a = net
    g = grads if extra else {"dscore": grads["dscore"]}
    loss = (a["Score"] * torch.as_tensor(g["dscore"])).sum()
    if extra:
        loss = loss + (a["Prob"] * torch.as_tensor(g["dprob"])).sum() + (a["Local_Fea"] * torch.as_tensor(g["dlocal_fea"])).sum() \
            + (a["Fea_Global"] * torch.as_tensor(g["dfea_global"])).sum()
    names = sorted(tw)
    want = torch.autograd.grad(loss, tp + [tw[n] for n in names], retain_graph=True)
    dpools, dparams = ref.walk(_acts(a), hw, **g)
    assert set(dparams) == set(names) and len(dparams) == 30
    for k in range(5):
        assert rel(dpools[k], want[k].numpy()) <= TOL, k
    for n, w in zip(names, want[5:]):
        assert dparams[n].shape == hw[n].shape and rel(dparams[n], w.numpy()) <= TOL, n
    # the torch walk (the GPU tests' yardstick, there in float32) is the same map
    tpools, tparams = ref.torch_walk(_acts(a), hw, dtype=F64, **g)
    assert all(rel(tpools[k], dpools[k]) <= TOL for k in range(5))
    assert all(rel(tparams[n], dparams[n]) <= TOL for n in names)


def test_central_finite_difference_of_a_directional_derivative(net):
    hw, pools, grads, tp, tw, a = net
    rng = np.random.default_rng(12)
    dpools, dparams = ref.walk(_acts(a), hw, grads["dscore"])
    dirs_p = [rng.standard_normal(p.shape) for p in pools]
    dirs_w = {n: rng.standard_normal(v.shape) * np.abs(v).max() for n, v in hw.items()}
    analytic = sum(np.vdot(d, g) for d, g in zip(dirs_p, dpools)) + sum(np.vdot(dirs_w[n], dparams[n]) for n in hw)

    # The backward is the derivative at FIXED gates, so the function differenced keeps every ReLU's mask: it is smooth (multilinear in
    # the variables), and no unit among the 10^6 that sits within eps of its kink can enter the difference.
    gates = ref.gates_of({k: v.detach() for k, v in a.items() if k != "pools"})

    def f(eps):
        with torch.no_grad():
            out = ref.torch_forward([torch.as_tensor(p + eps * d) for p, d in zip(pools, dirs_p)],
                                    {n: torch.as_tensor(v + eps * dirs_w[n]) for n, v in hw.items()}, gates)
        return float((out["Score"] * torch.as_tensor(grads["dscore"])).sum())

    eps = 1e-5
    fd = (f(eps) - f(-eps)) / (2 * eps)
    print(f"directional derivative: analytic {analytic:.10e} finite difference {fd:.10e}")
    # central difference: O(eps^2) truncation; cancellation of a 1.2e5-term float64 sum, about 1e-11 / eps = 1e-6 absolute
    assert abs(fd - analytic) <= 1e-5 * max(abs(analytic), 1.0)
