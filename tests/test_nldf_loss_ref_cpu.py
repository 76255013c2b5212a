"""tests/nldf_loss_ref.py, the numpy restatement of NLDF's objective (NLDF.py:79-100, :136-171) that the GPU tests measure against:
checked against an independent torch float64 composition (values, and the gradient through torch.autograd), by finite differences,
against np.pad's SYMMETRIC mode, and on hand-derived answers."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import nldf_loss_ref as ref

RTOL = 1e-12


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _torch_im_gradient(x):
    """x [B,H,W,C] float64: replicate pad, depthwise conv2d with the two Sobel filters, magnitude."""
    C = x.shape[3]
    fx = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]], dtype=torch.float64)
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate")
    gx = F.conv2d(xp, fx.expand(C, 1, 3, 3).contiguous(), groups=C)
    gy = F.conv2d(xp, fx.t().expand(C, 1, 3, 3).contiguous(), groups=C)
    return torch.sqrt(gx * gx + gy * gy).permute(0, 2, 3, 1)


def _torch_loss(score, label, th=1.5):
    P = torch.softmax(score, dim=-1)
    pg = torch.tanh(_torch_im_gradient(P).sum(dim=-1, keepdim=True))
    lg = (_torch_im_gradient(label).sum(dim=-1, keepdim=True) > th).double()
    iou = 1 - 2 * ((pg * lg).sum() + 1) / ((pg * pg).sum() + (lg * lg).sum() + 1)
    ce = (-(label * torch.log_softmax(score, dim=-1)).sum(dim=-1)).mean()
    return iou + ce, iou, ce, pg, lg


def _inputs(B, H, W, seed, soft=False):
    rng = np.random.default_rng(seed)
    score = rng.standard_normal((B, H, W, 2)) * 2.0
    if soft:
        a = rng.random((B, H, W))
    else:
        a = (rng.random((B, H, W)) < 0.5).astype(np.float64)
    return score, np.stack((a, 1.0 - a), axis=-1)


@pytest.mark.parametrize("B,H,W,soft", [(2, 5, 7, False), (1, 6, 4, True), (1, 1, 5, False), (2, 3, 1, False)])
def test_matches_torch_float64_composition(B, H, W, soft):
    score, label = _inputs(B, H, W, 10 * H + W, soft)
    assert ref.im_gradient(ref.softmax(score)).min() > 0 or H == 1 or W == 1      # no interior zero magnitude: the gradients agree
    ts = torch.from_numpy(score).requires_grad_(True)
    loss, iou, ce, pg, lg = _torch_loss(ts, torch.from_numpy(label))
    r = ref.saliency_loss(score, label)
    assert _rel(r["Loss_Mean"], loss.item()) <= RTOL and _rel(r["C_IoU_LOSS"], iou.item()) <= RTOL and _rel(r["CE"], ce.item()) <= RTOL
    assert _rel(r["Prob_Grad"], pg.detach().numpy()) <= RTOL
    assert np.array_equal(r["label_Grad"], lg.numpy())
    if H > 1 and W > 1:                              # a one-pixel axis has gy (or gx) == 0 everywhere; torch's sqrt then gives NaN
        loss.backward()
        assert _rel(ref.saliency_loss_grad(score, label), ts.grad.numpy()) <= RTOL


@pytest.mark.parametrize("C", [1, 2, 4])
def test_im_gradient_and_its_gradient_match_torch(C):
    rng = np.random.default_rng(C)
    x, g = rng.standard_normal((2, 5, 6, C)), rng.standard_normal((2, 5, 6, C))
    tx = torch.from_numpy(x).requires_grad_(True)
    out = _torch_im_gradient(tx)
    assert _rel(ref.im_gradient(x), out.detach().numpy()) <= RTOL
    out.backward(torch.from_numpy(g))
    assert _rel(ref.im_gradient_grad(x, g), tx.grad.numpy()) <= RTOL


def test_scalar_losses_match_torch():
    rng = np.random.default_rng(5)
    pred, gt = rng.random(255) * 0.98 + 0.01, (rng.random(255) < 0.3).astype(np.float64)
    tp, tg = torch.from_numpy(pred).requires_grad_(True), torch.from_numpy(gt)
    iou = 1 - 2 * ((tp * tg).sum() + 1) / ((tp * tp).sum() + (tg * tg).sum() + 1)
    con = (-tg * torch.log(tp + 1e-5) - (1 - tg) * torch.log(1 - tp + 1e-5)).mean()
    l2 = 0.0005 * (tp * tp).sum() / 2
    for value, grad, t in ((ref.loss_iou(pred, gt), ref.loss_iou_grad(pred, gt), iou),
                           (ref.loss_contour(pred, gt), ref.loss_contour_grad(pred, gt), con),
                           (ref.l2(pred, 0.0005), ref.l2_grad(pred, 0.0005), l2)):
        tp.grad = None
        t.backward()
        assert _rel(value, t.item()) <= RTOL and _rel(grad, tp.grad.numpy()) <= RTOL


def test_dscore_by_finite_differences():
    B, H, W = 1, 3, 4
    score, label = _inputs(B, H, W, 3)
    label[0, :, :2] = (1.0, 0.0)
    label[0, :, 2:] = (0.0, 1.0)                      # one vertical edge: label_Grad has ones and zeros
    assert 0 < ref.saliency_loss(score, label)["label_Grad"].sum() < H * W
    g = ref.saliency_loss_grad(score, label)
    h = 1e-6
    for idx in np.ndindex(B, H, W, 2):
        up, dn = score.copy(), score.copy()
        up[idx] += h
        dn[idx] -= h
        fd = (ref.saliency_loss(up, label)["Loss_Mean"] - ref.saliency_loss(dn, label)["Loss_Mean"]) / (2 * h)
        assert abs(fd - g[idx]) <= 1e-8 + 1e-6 * abs(g[idx]), (idx, fd, g[idx])


@pytest.mark.parametrize("shape", [(1, 4, 5, 2), (2, 1, 6, 2), (1, 3, 1, 1), (1, 1, 1, 2)])
def test_clamp_is_symmetric_pad_of_one(shape):
    x = np.random.default_rng(1).standard_normal(shape)
    assert np.array_equal(ref.pad1(x), np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="symmetric"))


def test_known_answer_vertical_edge():
    """4x4 one-hot label, class 0 in columns 0-1 and class 1 in columns 2-3.  Per channel gx = +-4 in columns 1 and 2 (the three rows'
    weights 1 + 2 + 1 on a step of 1, also at the clamped top and bottom rows) and 0 in columns 0 and 3 (the clamp repeats the edge
    pixel); gy = 0.  The summed magnitude is 2 sqrt(a^2 + b^2) = 8 or 0, never near 1.5."""
    label = np.zeros((1, 4, 4, 2))
    label[0, :, :2, 0] = 1.0
    label[0, :, 2:, 1] = 1.0
    want_sum = np.array([[0., 8., 8., 0.]] * 4)
    want = np.array([[0., 1., 1., 0.],
                     [0., 1., 1., 0.],
                     [0., 1., 1., 0.],
                     [0., 1., 1., 0.]])
    for dt in (np.float64, np.float32):
        assert np.array_equal(ref.label_grad_sum(label, dt)[0, :, :, 0], want_sum)
        score = np.zeros((1, 4, 4, 2))
        r = ref.saliency_loss(score, label, dtype=dt)
        assert np.array_equal(r["label_Grad"][0, :, :, 0], want)
        # a flat score: P = 1/2 everywhere, Prob_Grad = 0, I = 0, U = 8: C_IoU_LOSS = 1 - 2/9; CE = log 2
        assert abs(r["C_IoU_LOSS"] - (1 - 2 / 9)) <= 1e-6 and abs(r["CE"] - np.log(2.0)) <= 1e-6
        assert r["correct"] == 8 and r["accuracy"] == 0.5                 # every tie goes to channel 0: right in columns 0-1
    assert ref.loss_iou(want, want) == 1 - 2 * 9 / 17                       # I = 8, U = 16


def test_one_hot_label_sums_are_zero_or_at_least_two():
    rng = np.random.default_rng(9)
    a = (rng.random((3, 9, 11)) < 0.5).astype(np.float64)
    s = ref.label_grad_sum(np.stack((a, 1 - a), axis=-1))
    assert np.all((s == 0) | (s >= 2))
    s32 = ref.label_grad_sum(np.stack((a, 1 - a), axis=-1), np.float32)
    assert np.all((s32 == 0) | (s32 >= 2)) and np.array_equal(s > 1.5, s32 > 1.5)                # the threshold is exact in float32 too


def test_zero_magnitude_passes_no_gradient():
    score = np.zeros((1, 4, 6, 2))
    score[..., 0] = 200.0
    score[:, :, 3:, :] = (-200.0, 200.0)              # saturated: P is exactly (1, 0) | (0, 1)
    label = np.zeros_like(score)
    label[..., 0] = 1.0
    g = ref.saliency_loss_grad(score, label)
    assert np.all(np.isfinite(g))
    assert np.array_equal(ref.im_gradient_grad(np.zeros((1, 3, 3, 1)), np.ones((1, 3, 3, 1))), np.zeros((1, 3, 3, 1)))


def test_sobel_filter_literal():
    fx, fy = ref.sobel_filter()
    assert fx.shape == fy.shape == (3, 3, 2, 1) and fx.dtype == np.float32
    for c in range(2):
        assert fx[:, :, c, 0].tolist() == [[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]]
        assert fy[:, :, c, 0].tolist() == [[-1, -2, -1], [0, 0, 0], [1, 2, 1]]
