"""tests/vgg_grad_ref.py, the float64 reference of the VGG16 backward, checked on the CPU: against torch.autograd in float64, against a
central finite difference, and on the hand-made plane of the tie and zero rules."""
import functools

import numpy as np
import torch

from tests import vgg_grad_ref as ref

B, H, W = 2, 10, 14              # odd at every pool level: 5x7, 3x4, 2x2, 1x1, 1x1


@functools.lru_cache(maxsize=None)
def problem():
    rng = np.random.default_rng(11)
    params = {name: [rng.standard_normal((3, 3, ci, co)) * np.sqrt(2.0 / (9 * ci)), rng.standard_normal(co) * 0.05]
              for name, ci, co, _ in ref.LAYERS}
    x = rng.standard_normal((B, H, W, 3))
    outs = ref.forward(x, params)
    grads = {n: rng.standard_normal(outs[ref.OUTPUTS.index(n)].shape) for n in ("pool1", "conv3_2", "pool3", "pool5")}
    return x, params, outs, grads


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def test_reference_matches_torch_autograd_in_float64():
    x, params, outs, grads = problem()
    dx, dparams = ref.backward(x, params, grads, outs)
    tdx, tparams, touts = ref.torch_backward(x, params, grads, torch.float64)
    for o, t in zip(outs, touts):
        assert rel(o, t) < 1e-12
    assert rel(dx, tdx) < 1e-11
    for name, _, _, _ in ref.LAYERS:
        assert rel(dparams[name][0], tparams[name][0]) < 1e-11, name
        assert rel(dparams[name][1], tparams[name][1]) < 1e-11, name


def test_reference_matches_a_central_finite_difference():
    x, params, outs, grads = problem()
    dx, dparams = ref.backward(x, params, grads, outs)
    rng = np.random.default_rng(3)
    vx = rng.standard_normal(x.shape)
    # a direction of the parameters' own scale: the loss is a polynomial of degree 13 in the filters, whose curvature along a
    # direction a hundred times larger than they are would swamp the difference quotient
    vW = {n: (rng.standard_normal(p[0].shape) * p[0].std(), rng.standard_normal(p[1].shape) * p[1].std()) for n, p in params.items()}

    def loss(t):
        o = ref.forward(x + t * vx, {n: [p[0] + t * vW[n][0], p[1] + t * vW[n][1]] for n, p in params.items()})
        return sum(float((o[ref.OUTPUTS.index(n)] * g).sum()) for n, g in grads.items())

    want = float((dx * vx).sum()) + sum(float((dparams[n][0] * vW[n][0]).sum() + (dparams[n][1] * vW[n][1]).sum()) for n in params)
    eps = 1e-6
    got = (loss(eps) - loss(-eps)) / (2 * eps)
    assert abs(got - want) <= 1e-5 * abs(want), (got, want)


def test_tie_rule_and_zero_rule_on_the_hand_made_plane():
    y, dpool, dy = ref.tie_plane()
    got = ref.pool_relu_backward(y[None, :, :, None], dpool[None, :, :, None])[0, :, :, 0]
    assert np.array_equal(got, dy)
    assert np.array_equal(ref.pool_forward(y[None, :, :, None])[0, :, :, 0], np.array([[5., 2.], [0., 3.]]))


def test_gradient_below_the_deepest_output_only():
    x, params, outs, _ = problem()
    g = np.ones_like(outs[ref.OUTPUTS.index("pool2")])
    dx, dparams = ref.backward(x, params, {"pool2": g}, outs)
    assert np.abs(dx).max() > 0
    for name, _, _, _ in ref.LAYERS[4:]:
        assert not dparams[name][0].any() and not dparams[name][1].any()
