"""`train_step.Trainer` at sizes that are no multiple of 64: decoder levels that are NOT twice the level below them.  There the
transposed convolutions are cropped to their skip size, the 3x3 Winograd stages have a ragged last tile row / column, the 2x bilinear
residuals run between sizes that are not in ratio 2, and the full-resolution head gathers from a concat2 that is no clean quarter of
the frame.  The kernels have their own tests at such sizes (test_gpu_train_conv_edges.py, test_gpu_training.py); what is checked here
is that train_step.py wires them together: forty buffers sized from the level table, the heads' gather geometry, the
overwrite-then-accumulate order of the activation gradients on cropped buffers.

Method and every bound: tests/train_step_check.py, i.e. those of test_gpu_train_step.py at 192x256.  The shapes (pinned, with what each
reaches, by tests/test_train_step_shapes_cpu.py) keep at least 32 rows in the coarsest BatchNorm.  Each case prints its largest
relative gradient error and the form, Winograd or direct, that every 3x3 stride-1 stage took (pytest -s)."""
import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import train_step, weights as wts
from oracle import vstab_oracle as vo
from tests.train_step_check import ODD_SHAPES, check_network_backward

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("winograd", [False, True], ids=["direct", "winograd"])
@pytest.mark.parametrize("B,H,W", ODD_SHAPES, ids=[f"{b}x{h}x{w}" for b, h, w in ODD_SHAPES])
def test_network_backward_matches_autograd_at_odd_level_sizes(B, H, W, winograd):
    case = check_network_backward(B, H, W, winograd)
    tr, R = case.tr, {k: v.cuda() for k, v in case.R.items()}

    # padding stays zero: the pad channels of every parameter gradient, the two pad channels of every flow gradient
    for k, t in tr.g.items():
        mask = torch.ones_like(t, dtype=torch.bool)
        mask[tuple(slice(0, s) for s in tr.shape_real[k])] = False
        if mask.any():
            assert float(t[mask].abs().max()) == 0.0, k
    for level, d in tr.dpf.items():
        assert tuple(d.shape[1:3]) == tuple(case.oracle[level].shape[1:3])
        assert float(d[..., 2:].abs().max()) == 0.0, level

    # no stale state: the activation gradients are never cleared -- the first write of a backward pass into each buffer overwrites,
    # later ones accumulate -- so a row or column that a crop discards must receive nothing and keep nothing.  Another batch and
    # other upstream gradients in between, then the first pass again: bit for bit the same gradients.
    first = {k: t.clone() for k, t in tr.g.items()}
    g1 = torch.Generator().manual_seed(1000 + W)
    feats2 = torch.rand(B, H, W, 27, generator=g1) * 2.0 - 0.5
    R2 = {k: (torch.randn(v.shape, generator=g1) * 3.0).cuda() for k, v in case.R.items()}
    tr.forward(feats2.cuda())
    tr.backward_from_flow_grads(R2)
    assert any(not torch.equal(tr.g[k], first[k]) for k in first)          # (the pass in between did write other gradients)
    tr.forward(case.feats.cuda())
    tr.backward_from_flow_grads(R)
    stale = [k for k in train_step.Trainer._backward_order() if not torch.equal(tr.g[k], first[k])]
    assert not stale, stale


# ----------------------------------------------------------------------------- the step and the public entry at one odd size
OB, OH, OW = 2, 194, 258


def test_loss_adam_and_padding_at_an_odd_size():
    """test_loss_adam_and_padding of test_gpu_train_step.py at 194x258 (every decoder level cropped on both axes)"""
    B, H, W = OB, OH, OW
    w = wts.synthetic_weights(seed=12, cin=27, random_bn=True, flow_gain=0.5)
    g0 = torch.Generator().manual_seed(H)
    feats = torch.rand(B, H, W, 27, generator=g0)
    gt, un = torch.rand(B, H, W, 3, generator=g0), torch.rand(B, H, W, 3, generator=g0)
    tr = train_step.Trainer(w, B, H, W)
    flows = tr.forward(feats.cuda())
    # loss_main of the oracle on the SAME flows (the loss kernels' own parity test covers value and gradient)
    ref_loss = float(vo.loss_main({k: v.float().cpu() for k, v in flows.items()}, gt, un))
    loss = tr.loss_and_backward(gt.cuda(), un.cuda())
    assert abs(float(loss) - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss))
    got = tr.export(tr.g)
    assert len(got) == 60
    assert all(np.isfinite(v).all() for v in got.values())
    assert max(float(np.abs(v).max()) for v in got.values()) > 0
    # one Adam update from those gradients (t = 1: lr_t = lr * sqrt(1 - b2) / (1 - b1))
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    before = tr.export()
    tr.adam(lr, b1, b2, eps)
    after = tr.export()
    for k, g in got.items():
        g64 = g.astype(np.float64)
        m, v = (1 - b1) * g64, (1 - b2) * g64 * g64
        exp = before[k].astype(np.float64) - lr * np.sqrt(1 - b2) / (1 - b1) * m / (np.sqrt(v) + eps)
        assert np.abs(after[k] - exp).max() <= 1e-6 + 1e-5 * np.abs(exp).max(), k
    # the zero padding of the stored parameters survives the update
    for k, t in tr.p.items():
        mask = torch.ones_like(t, dtype=torch.bool)
        mask[tuple(slice(0, s) for s in tr.shape_real[k])] = False
        if mask.any():
            assert float(t[mask].abs().max()) == 0.0, k


def test_flownetS_pyramid_is_train_true_and_sync_back_at_an_odd_size():
    """test_flownetS_pyramid_is_train_true_and_sync_back at 194x258: the inference path at odd sizes has its own tests, the hand-over
    from a Trainer built at one does not"""
    import coupe.optical_flow_based_deep_video_stabilization_amd as vs
    from coupe.optical_flow_based_deep_video_stabilization_amd import runtime
    B, H, W = OB, OH, OW
    runtime.reset()
    w = vs.initialize_global_variables(seed=4, cin=27, random_bn=True, flow_gain=0.3)
    g0 = torch.Generator().manual_seed(7)
    feats = torch.rand(B, H, W, 27, generator=g0).cuda()
    out = vs.flownetS_pyramid(feats, B, is_train=True)
    ref = vo.flownetS_pyramid(feats.cpu(), w, dtype=torch.float64, is_train=True)
    assert set(out) == {"predict_flow6", "predict_flow5", "predict_flow4", "predict_flow3", "predict_flow2", "flow"}
    for k in vo.LOSS_LEVELS:
        assert out[k].shape == ref[k].shape and out[k].is_contiguous()
        assert float((out[k].double().cpu() - ref[k]).abs().max()) <= 2e-3
    tr = train_step.get_trainer("flownetS", B, H, W)
    assert tr is train_step.get_trainer("flownetS", B, H, W)
    assert (tr.H, tr.W) == (H, W) and tr.hw["concat2"] == (49, 65)
    gt, un = torch.rand(B, H, W, 3, generator=g0).cuda(), torch.rand(B, H, W, 3, generator=g0).cuda()
    tr.step(feats, gt, un, lr=1e-4)
    train_step.sync_to_inference(tr)
    inf = vs.flownetS_pyramid(feats, B, is_train=False)
    ref2 = vo.flownetS_pyramid(feats.cpu(), tr.export(), dtype=torch.float64)
    assert inf["predict_flow2"].shape == ref2["predict_flow2"].shape
    assert float((inf["predict_flow2"].double().cpu() - ref2["predict_flow2"]).abs().max()) <= 1e-3
