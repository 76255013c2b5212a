"""The shared body of the network-level checks of `train_step.Trainer` (tests/test_gpu_train_step.py at 192x256,
tests/test_gpu_train_step_odd_sizes.py at sizes whose decoder levels are cropped and whose Winograd tile grids are ragged): one
train-mode forward and one backward pass from FIXED upstream flow gradients against the fp64 oracle under torch autograd.

Why the oracle is run with the implementation's own leaky-relu pattern and why the upstream gradients are fixed is told in
tests/test_gpu_train_step.py.  Every bound here is that test's; nothing is derived per shape.

`ODD_SHAPES` is pinned by tests/test_train_step_shapes_cpu.py (level sizes, which decoder levels crop, rows at conv6_1)."""
import functools
import types

import numpy as np
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import train_step, weights as wts
from oracle import vstab_oracle as vo

BN_LAYERS = [e[0] for e in train_step.ENC] + ["deconv5", "deconv4", "deconv3", "deconv2"]
WINO_STAGES = [e[0] for e in train_step.ENC if e[1] == 3 and e[2] == 1]       # 3_1, 4_1, 5_1, 6_1
# (B, H, W) whose level sizes are no multiple of each other: see the table in tests/test_train_step_shapes_cpu.py
ODD_SHAPES = ((2, 194, 258), (2, 200, 264), (3, 131, 197))
WEIGHT_SEED = 13


def inputs(B, H, W, weight_seed=WEIGHT_SEED):
    """(weights, generator, features) exactly as test_network_backward_matches_autograd always drew them"""
    w = wts.synthetic_weights(seed=weight_seed, cin=27, random_bn=True, flow_gain=0.5)
    g0 = torch.Generator().manual_seed(H)
    feats = torch.rand(B, H, W, 27, generator=g0)
    return w, g0, feats


@functools.lru_cache(maxsize=None)
def _own_pattern_oracle(B, H, W, weight_seed):
    """The fp64 oracle's internals on ITS OWN activation pattern: the same for the Winograd and the direct case of a shape"""
    w, _g0, feats = inputs(B, H, W, weight_seed)
    with torch.no_grad():
        _, own = vo.flownetS_pyramid(feats, w, torch.float64, return_internals=True, is_train=True)
    return own


def record_forms(tr):
    """Wrap the Trainer's two Winograd gates so that the form every 3x3 stride-1 stage actually took is on record:
    returns {"forward" | "dgrad" | "wgrad": [took Winograd, ...] in call order}."""
    rec = {"forward": [], "dgrad": [], "wgrad": []}
    wino, wino_wgrad, rowwin = tr._wino, tr._wino_wgrad, tr._conv1_rowwin
    tr.conv1_rowwin = []                                      # and whether conv1 ran on the row-window kernel (it declines some widths)

    def _wino(x, cx_off, W, transpose, bias, y, cy_off, act):
        took = wino(x, cx_off, W, transpose, bias, y, cy_off, act)
        rec["dgrad" if transpose else "forward"].append(bool(took))
        return took

    def _wino_wgrad(*a):
        took = wino_wgrad(*a)
        rec["wgrad"].append(bool(took))
        return took

    def _conv1_rowwin(*a):
        took = rowwin(*a)
        tr.conv1_rowwin.append(bool(took))
        return took

    tr._wino, tr._wino_wgrad, tr._conv1_rowwin = _wino, _wino_wgrad, _conv1_rowwin
    return rec


def forms_by_stage(rec):
    """{stage: {"forward": bool, "dgrad": bool, "wgrad": bool}} of ONE forward and ONE backward pass (the forward visits the stages
    in encoder order, the backward pass last stage first)"""
    assert all(len(v) == len(WINO_STAGES) for v in rec.values()), rec
    order = {"forward": WINO_STAGES, "dgrad": WINO_STAGES[::-1], "wgrad": WINO_STAGES[::-1]}
    return {s: {kind: rec[kind][order[kind].index(s)] for kind in rec} for s in WINO_STAGES}


def check_network_backward(B, H, W, winograd, weight_seed=WEIGHT_SEED):
    """Forward, activation pattern, all 60 gradients and the moving statistics of one Trainer at B x H x W against the oracle.
    Returns what the checks were made of (Trainer, inputs, oracle flows, upstream gradients, both gradient sets, the forms taken)
    for the callers that check more."""
    w, g0, feats = inputs(B, H, W, weight_seed)
    tr = train_step.Trainer(w, B, H, W)
    tr.wino_min_flops = 0.0 if winograd else 1e30          # force / forbid the Winograd form of the 3x3 stride-1 stages
    rec = record_forms(tr)
    flows = tr.forward(feats.cuda())

    # The activation pattern itself (the gradient check below feeds the implementation's own leaky-relu
    # sides to the oracle): against the fp64 oracle run on ITS OWN pattern, an element may sit on the other side of the kink
    # only if its value is within rounding distance of zero, and only a handful may at all.
    masks = tr.lrelu_masks()
    own = _own_pattern_oracle(B, H, W, weight_seed)
    enc_names = [e[0] for e in train_step.ENC]
    for name in enc_names + ["deconv5", "deconv4", "deconv3", "deconv2"]:
        if name in enc_names:
            y = own[f"conv{name}"]
            m = masks[name]
        else:
            cat = own["concat" + name[-1]]                         # [skip | deconvN | upsampled flow]
            skip = {"5": 512, "4": 512, "3": 256, "2": 128}[name[-1]]
            y = cat[..., skip:cat.shape[3] - 2]
            m = masks[name + "_bn"]
        flips = (y > 0) != m
        nflip = int(flips.sum())
        assert nflip <= max(4, int(2e-4 * y.numel())), (name, nflip, y.numel())
        if nflip:
            assert float(y[flips].abs().max()) <= 2e-4 * max(1.0, float(y.abs().max())), (name, float(y[flips].abs().max()))

    Wt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=("moving_" not in k)) for k, v in w.items()}
    stats = {}
    out = vo.flownetS_pyramid(feats, Wt, is_train=True, batch_stats=stats, lrelu_masks=masks)
    for k in vo.LOSS_LEVELS:                                   # train-mode forward (batch statistics)
        assert tuple(flows[k].shape) == tuple(out[k].shape), (k, tuple(flows[k].shape), tuple(out[k].shape))
        assert float((flows[k].double().cpu() - out[k].detach()).abs().max()) <= 2e-3, k
    R = {k: torch.randn(out[k].shape, generator=g0) for k in vo.LOSS_LEVELS}
    sum((out[k] * R[k].double()).sum() for k in vo.LOSS_LEVELS).backward()
    ref = {k: v.grad for k, v in Wt.items() if v.grad is not None}

    tr.backward_from_flow_grads({k: v.cuda() for k, v in R.items()})
    forms = forms_by_stage(rec)
    if not winograd:                                           # (a forced stage may still decline its geometry: printed below)
        assert not any(took for stage in forms.values() for took in stage.values()), forms
    got = tr.export(tr.g)
    assert set(got) == set(ref) and len(ref) == 60
    # every tensor is compared before anything is reported, in the order the backward pass finishes them: the first name in
    # the report is the stage that broke, what follows it is downstream of it
    failures, worst = [], (0.0, None)
    order = train_step.Trainer._backward_order()
    assert set(order) == set(ref)
    for k in order:
        r = ref[k]
        d = float((torch.from_numpy(got[k]).double() - r).abs().max())
        layer, leaf = k.split("/")
        if leaf in ("b_conv2d", "b_deconv2d") and layer in BN_LAYERS:
            # a bias in front of BatchNorm has an exactly-zero gradient (the mean subtraction removes it): the computed
            # value is rounding noise of the sum of dz, measured against the size of the layer's beta gradient
            beta = ref[(layer if leaf == "b_conv2d" else layer + "_bn") + "/beta"]
            if not (float(r.abs().max()) < 1e-6 and d <= 1e-3 * float(beta.abs().max())):
                failures.append((k, d, float(r.abs().max())))
        else:
            if not d <= 1e-4 * float(r.abs().max()) + 1e-9:
                failures.append((k, d, float(r.abs().max())))
            rel = d / float(r.abs().max()) if float(r.abs().max()) > 0 else float("inf")
            if worst[1] is None or rel > worst[0]:
                worst = (rel, k)
    print(f"[train-step {B}x{H}x{W} winograd={winograd}] largest gradient error / max|ref| {worst[0]:.3e} on {worst[1]}; conv1 "
          f"{'row-window' if tr.conv1_rowwin[0] else 'tiled'}; forms "
          + ", ".join(f"conv{s}: " + "/".join(f"{kind} {'winograd' if took else 'direct'}" for kind, took in forms[s].items())
                      for s in WINO_STAGES))
    assert not failures, "gradients off, in backward order (name, max error, max|ref|):\n" + "\n".join(
        f"  {k}: {d:.3e} against {r:.3e}" for k, d, r in failures)

    # BatchNorm moving averages after this ONE forward (TensorLayer: decay 0.9)
    newp = tr.export()
    for name, (m, v) in stats.items():
        mm = w[f"{name}/moving_mean"].astype(np.float64) * 0.9 + m.numpy() * 0.1
        mv = w[f"{name}/moving_variance"].astype(np.float64) * 0.9 + v.numpy() * 0.1
        assert np.abs(newp[f"{name}/moving_mean"] - mm).max() <= 1e-4 * max(1.0, np.abs(mm).max()), name
        assert np.abs(newp[f"{name}/moving_variance"] - mv).max() <= 1e-3 * max(1.0, np.abs(mv).max()), name
    return types.SimpleNamespace(tr=tr, w=w, gen=g0, feats=feats, flows=flows, oracle=out, R=R, ref=ref, got=got, forms=forms,
                                 record=rec, worst=worst)
