"""The objective with the previous-frame terms (main_flownetS_pyramid.py:200-250 and the highTV file) on the GPU:
`vstab_loss_level_multi` / `vstab_loss_main_multi`, `training.lossterm_multi` / `loss_main_multi` and `Trainer(objective=...)` against
the one-target entry points (bit for bit: two ABI paths onto one kernel pair) and against the fp64 reference of
tests/loss_prev_ref.py (bounds stated there).  Shapes are those of test_gpu_training.py: the last level of the first case crosses one
4096-pixel workgroup of pass 1."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime, train_step, training, weights as wts
from coupe.optical_flow_based_deep_video_stabilization_amd.warp_flow import resize_images
from oracle import vstab_oracle as vo
from tests import loss_prev_ref as ref

pytestmark = pytest.mark.gpu

CASES = [(2, 64, 96, [(1, 2), (2, 3), (4, 6), (8, 12), (62, 94)]),
         (1, 48, 64, [(1, 1), (2, 2), (3, 4), (6, 8), (46, 62)]),
         (3, 40, 40, [(1, 1), (2, 2), (3, 3), (5, 5), (38, 38)])]
PREV = {"prev": training.OBJECTIVE_PREV, "prev_hightv": training.OBJECTIVE_PREV_HIGHTV}
LEVELS = vo.LOSS_LEVELS


@functools.lru_cache(maxsize=None)
def _case(i):
    """Inputs of case i and the fp64 pieces every objective over the six targets is assembled from: computed once, shared, not modified."""
    B, H, W, sizes = CASES[i]
    stab, un, flows = ref.case(B, H, W, sizes, seed=B * 7 + H)
    return stab, un, flows, ref.pieces(flows, stab, un, training.OBJECTIVE_PREV.target_channels)


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _level_multi_raw(pf, G, U, c_off, weights, scale_tv, need_grad=True):
    """vstab_loss_level_multi on resized inputs -> (rc, sums [B,T+2], grad or None)."""
    B, h, w, _ = pf.shape
    T = len(c_off)
    sums = torch.full(((T + 2) * B,), -1.0, dtype=torch.float64, device=pf.device)
    grad = torch.full_like(pf, 7.0) if need_grad else None
    rc = _lib.lib().vstab_loss_level_multi(pf.data_ptr(), G.data_ptr(), G.shape[3], T, (C.c_int32 * T)(*c_off), (C.c_float * T)(*weights),
                                           U.data_ptr(), B, h, w, sums.data_ptr(), scale_tv, grad.data_ptr() if need_grad else None,
                                           runtime.stream_ptr())
    return rc, sums.view(B, T + 2), grad


def _check_against_reference(loss, per, grads, p, obj, what=""):
    """Issue bounds: loss and per-target losses within 2e-5 * max(1, |ref|); every level's gradient within
    2e-5 * sum_t w_t * max|g_t_ref| + 1e-9, g_t_ref the reference gradient of target t's term alone (TV counted once, in t = 0)."""
    rloss, rper, rgrads = ref.assemble(p, obj)
    tg = ref.term_gradients(p, obj)
    print(f"{what} loss {float(loss):.9g} ref {rloss:.9g}")
    assert abs(float(loss) - rloss) <= 2e-5 * max(1.0, abs(rloss))
    for t, (a, b) in enumerate(zip(per.cpu().tolist(), rper)):
        assert abs(a - b) <= 2e-5 * max(1.0, abs(b)), (t, a, b)
    for k in LEVELS:
        g = grads[k].double().cpu()
        assert g.shape == rgrads[k].shape and bool(torch.isfinite(g).all())
        err, tol = float((g - rgrads[k]).abs().max()), ref.gradient_bound(tg[k], obj)
        print(f"{what} {k}: max err {err:.3e} bound {tol:.3e}")
        assert err <= tol, (k, err, tol)


# ----------------------------------------------------------------------------- 1. one target, weight 1: vstab_loss_level bit for bit
@pytest.mark.parametrize("i", range(len(CASES)))
def test_one_target_weight_one_is_loss_level_bit_for_bit(i):
    stab, un, flows, _p = _case(i)
    L = _lib.lib()
    for c_off in (0, 6, 21):
        for name in LEVELS:
            pf = flows[name].cuda()
            B, h, w, _ = pf.shape
            G, U = resize_images(stab.cuda(), (h, w)), resize_images(un.cuda(), (h, w))
            g3 = G[..., c_off:c_off + 3].contiguous()
            sums0 = torch.empty(3 * B, dtype=torch.float64, device="cuda")
            grad0 = torch.empty_like(pf)
            _lib.check(L.vstab_loss_level(pf.data_ptr(), g3.data_ptr(), U.data_ptr(), B, h, w, sums0.data_ptr(), 1.0, 6e-8, grad0.data_ptr(),
                                          runtime.stream_ptr()))
            rc, sums1, grad1 = _level_multi_raw(pf, G, U, [c_off], [1.0], 6e-8)
            assert rc == 0
            assert torch.equal(sums1.reshape(-1), sums0), (name, c_off)
            assert torch.equal(grad1, grad0), (name, c_off)
            rc, sums2, _ = _level_multi_raw(pf, G, U, [c_off], [1.0], 6e-8, need_grad=False)       # value only: the same sums
            assert rc == 0 and torch.equal(sums2, sums1)


def test_every_target_count_sums_are_the_single_target_sums():
    """T = 1..8 instantiate eight kernel pairs: target t's numerator is the one-target kernel's on that slice; den and TV are shared."""
    stab, un, flows, _p = _case(0)
    pf = flows[LEVELS[-1]].cuda()
    h, w = pf.shape[1:3]
    G, U = resize_images(stab.cuda(), (h, w)), resize_images(un.cuda(), (h, w))
    offs = [0, 3, 6, 9, 12, 15, 18, 21]
    single = [_level_multi_raw(pf, G, U, [o], [1.0], 0.0)[1] for o in offs]
    for T in range(1, 9):
        rc, sums, grad = _level_multi_raw(pf, G, U, offs[:T], [0.5 ** t for t in range(T)], 0.0)
        assert rc == 0 and bool(torch.isfinite(grad).all())
        for t in range(T):
            assert torch.equal(sums[:, t], single[t][:, 0]), (T, t)
        assert torch.equal(sums[:, T:], single[0][:, 1:]), T


# ----------------------------------------------------------------------------- 2. one resize of the 24-channel tensor
@pytest.mark.parametrize("i", range(len(CASES)))
def test_resize_of_the_target_tensor_equals_the_slices_resized_one_by_one(i):
    stab, _un, flows, _p = _case(i)
    s = stab.cuda()
    for name in LEVELS:
        h, w = flows[name].shape[1:3]
        whole = resize_images(s, (h, w))
        for c in range(0, 24, 3):
            assert torch.equal(whole[..., c:c + 3], resize_images(s[..., c:c + 3].contiguous(), (h, w))), (name, c)


# ----------------------------------------------------------------------------- 3. value and gradient against the fp64 reference
@pytest.mark.parametrize("name", sorted(PREV))
@pytest.mark.parametrize("i", range(len(CASES)))
def test_value_and_gradients_against_the_reference(i, name):
    stab, un, flows, p = _case(i)
    obj = PREV[name]
    fl = _cuda(flows)
    grads = {k: torch.empty_like(v) for k, v in fl.items()}
    loss, per = training.loss_main_multi(fl, stab.cuda(), un.cuda(), obj, grads)
    _check_against_reference(loss, per, grads, p, obj, f"case {i} {name}")
    # the per-level wrapper: same numbers through vstab_loss_level_multi
    total, per_sum = 0.0, torch.zeros(6, dtype=torch.float64)
    for k, tvw in zip(LEVELS, obj.tv_weights):
        l, g, pt = training.lossterm_multi(fl[k], stab.cuda(), un.cuda(), obj.target_channels, obj.target_weights, tvw)
        assert torch.equal(g, grads[k]), k
        total += float(l)
        per_sum += pt.cpu()
    assert abs(total - float(loss)) <= 1e-9 * max(1.0, abs(float(loss)))
    assert float((per_sum - per.cpu()).abs().max()) <= 1e-9


# ----------------------------------------------------------------------------- 4. composition from six calls of the existing entry point
@pytest.mark.parametrize("name", sorted(PREV))
@pytest.mark.parametrize("i", range(len(CASES)))
def test_composition_of_six_loss_main_fused_calls(i, name):
    """loss_main_fused on target slice t gives lossterms_t + TV under today's TV_WEIGHTS.  The objective is sum_t w_t * lossterms_t + TV
    under its own weights, so sum_t w_t * (call t) carries (sum_t w_t) * TV_WEIGHTS too much and the objective's TV weights too little;
    the TV value and its gradient per level come from the existing kernel as well (zero images: the photometric part vanishes)."""
    stab, un, flows, p = _case(i)
    obj = PREV[name]
    fl = _cuda(flows)
    s, u = stab.cuda(), un.cuda()
    wsum = sum(obj.target_weights)
    loss_c = 0.0
    grads_c = {k: torch.zeros(v.shape, dtype=torch.float64) for k, v in flows.items()}
    per_c = []
    for c, wt in zip(obj.target_channels, obj.target_weights):
        g = {k: torch.empty_like(v) for k, v in fl.items()}
        l = float(training.loss_main_fused(fl, s[..., c:c + 3].contiguous(), u, g))
        loss_c += wt * l
        per_c.append(l)
        for k in LEVELS:
            grads_c[k] += wt * g[k].double().cpu()
    tv_all = 0.0
    for k, tv_old, tv_new in zip(LEVELS, training.TV_WEIGHTS, obj.tv_weights):
        z = torch.zeros(*flows[k].shape[:3], 3).cuda()
        tv, sign = training.lossterm(fl[k], z, z, tv_weight=1.0)
        loss_c += (tv_new - wsum * tv_old) * float(tv)
        tv_all += tv_old * float(tv)
        grads_c[k] += (tv_new - wsum * tv_old) * sign.double().cpu()
    grads = {k: torch.empty_like(v) for k, v in fl.items()}
    loss, per = training.loss_main_multi(fl, s, u, obj, grads)
    tg = ref.term_gradients(p, obj)
    rloss = ref.assemble(p, obj)[0]
    assert abs(float(loss) - loss_c) <= 2e-5 * max(1.0, abs(rloss))
    for t, v in enumerate(per.cpu().tolist()):
        assert abs(v - (per_c[t] - tv_all)) <= 2e-5 * max(1.0, abs(v)), t
    for k in LEVELS:
        err, tol = float((grads[k].double().cpu() - grads_c[k]).abs().max()), ref.gradient_bound(tg[k], obj)
        print(f"case {i} {name} {k}: fused vs composed max diff {err:.3e} bound {tol:.3e}")
        assert err <= tol, (k, err, tol)


def test_level4_has_no_tv_part():
    """var4 is left out of the sum (:250): with targets equal to the warped frame (all zero) the photometric gradient vanishes and level
    4's flow gradient is exactly zero, while the other levels carry their TV sign pattern."""
    B, H, W, sizes = CASES[0]
    _stab, _un, flows, _p = _case(0)
    fl = _cuda(flows)
    for obj in PREV.values():
        grads = {k: torch.full_like(v, 7.0) for k, v in fl.items()}
        loss, per = training.loss_main_multi(fl, torch.zeros(B, H, W, 24).cuda(), torch.zeros(B, H, W, 3).cuda(), obj, grads)
        assert float(grads["predict_flow4"].abs().max()) == 0.0
        assert float(per.abs().max()) == 0.0
        tv = sum(w * float(vo.total_variation(flows[k])) for w, k in zip(obj.tv_weights, LEVELS))
        assert abs(float(loss) - tv) <= 2e-5 * max(1.0, tv)
        for k, w in zip(LEVELS, obj.tv_weights):
            if k != "predict_flow4":
                g = grads[k].cpu()
                assert float(g.abs().max()) > 0.0
                assert bool(torch.all(torch.round(g / np.float32(w)) * np.float32(w) == g)), k      # integer multiples of the float32 weight


# ----------------------------------------------------------------------------- 5. edge cases
EDGE_SIZES = [(1, 2), (2, 3), (3, 4), (5, 6), (18, 22)]


def _edge_case(far_sample=None, zero=False):
    B, H, W = 2, 20, 24
    stab, un, flows = ref.case(B, H, W, EDGE_SIZES, seed=77)
    for k in flows:
        if zero:
            flows[k] = torch.zeros_like(flows[k])
        if far_sample is not None:
            flows[k][far_sample] = 1e4
    return stab, un, flows


def test_a_sample_whose_flow_lies_far_outside():
    stab, un, flows = _edge_case(far_sample=1)
    obj = training.OBJECTIVE_PREV
    fl = _cuda(flows)
    grads = {k: torch.empty_like(v) for k, v in fl.items()}
    loss, per = training.loss_main_multi(fl, stab.cuda(), un.cuda(), obj, grads)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(per).all())
    _check_against_reference(loss, per, grads, ref.pieces(flows, stab, un, obj.target_channels), obj, "far sample")
    for k in LEVELS:                                   # mask all zero: den = 3*h*w*1e-8 (the float32 1e-8 of safe(M)), numerators 0
        h, w = flows[k].shape[1:3]
        G, U = resize_images(stab.cuda(), (h, w)), resize_images(un.cuda(), (h, w))
        rc, sums, grad = _level_multi_raw(fl[k], G, U, list(obj.target_channels), list(obj.target_weights), 0.0)
        assert rc == 0
        assert abs(float(sums[1, 6]) - 3 * h * w * float(np.float32(1e-8))) <= 1e-12 * 3 * h * w * 1e-8
        assert float(sums[1, :6].abs().max()) == 0.0 and float(grad[1].abs().max()) == 0.0
        assert float(sums[0, 6]) > 1.0 or h * w < 4


def test_zero_flow():
    stab, un, flows = _edge_case(zero=True)
    obj = training.OBJECTIVE_PREV_HIGHTV
    fl = _cuda(flows)
    grads = {k: torch.empty_like(v) for k, v in fl.items()}
    loss, per = training.loss_main_multi(fl, stab.cuda(), un.cuda(), obj, grads)
    p = ref.pieces(flows, stab, un, obj.target_channels)
    assert all(v == 0.0 for v in p["tv"])
    for k in LEVELS:                                   # |q - f| at q == f: the kernel's sign(0) = 0 is the subgradient autograd picks too
        assert float(p["tv_grads"][k].abs().max()) == 0.0
    _check_against_reference(loss, per, grads, p, obj, "zero flow")


def test_value_only_strided_pixels_and_reproducibility():
    stab, un, flows, _p = _case(0)
    obj = training.OBJECTIVE_PREV
    fl, s, u = _cuda(flows), stab.cuda(), un.cuda()
    grads = {k: torch.empty_like(v) for k, v in fl.items()}
    loss, per = training.loss_main_multi(fl, s, u, obj, grads)
    loss0, per0 = training.loss_main_multi(fl, s, u, obj)                      # grads=None: value only
    assert abs(float(loss0) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float((per0 - per).abs().max()) <= 1e-12
    # flows inside 4-channel pixels, gradients into 4-channel pixels: channels 0..1 as above, the others untouched
    wide = {k: torch.zeros(*v.shape[:3], 4).cuda() for k, v in flows.items()}
    for k, v in fl.items():
        wide[k][..., :2] = v
    gw = {k: torch.full_like(v, 7.0) for k, v in wide.items()}
    loss_w, _ = training.loss_main_multi(wide, s, u, obj, gw)
    assert abs(float(loss_w) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    for k in LEVELS:
        assert torch.equal(gw[k][..., :2], grads[k]), k
        assert float((gw[k][..., 2:] - 7.0).abs().max()) == 0.0
    # a second run gives the same gradients bit for bit
    again = {k: torch.empty_like(v) for k, v in fl.items()}
    training.loss_main_multi(fl, s, u, obj, again)
    for k in LEVELS:
        assert torch.equal(again[k], grads[k]), k
    # a 12-channel stable tensor that holds the objective's first four targets is accepted
    small = training.Objective((0, 3, 6, 9), obj.target_weights[:4], obj.tv_weights)
    g12 = {k: torch.empty_like(v) for k, v in fl.items()}
    l12, _ = training.loss_main_multi(fl, s[..., :12].contiguous(), u, small, g12)
    g24 = {k: torch.empty_like(v) for k, v in fl.items()}
    l24, _ = training.loss_main_multi(fl, s, u, small, g24)
    assert abs(float(l12) - float(l24)) <= 1e-12 * max(1.0, abs(float(l24)))
    assert all(torch.equal(g12[k], g24[k]) for k in LEVELS)


# ----------------------------------------------------------------------------- 6. Trainer
def _trainer_inputs(seed):
    B, H, W = 2, 96, 128
    g0 = torch.Generator().manual_seed(seed)
    feats = torch.rand(B, H, W, 27, generator=g0).cuda()
    stab, un = torch.rand(B, H, W, 24, generator=g0).cuda(), torch.rand(B, H, W, 3, generator=g0).cuda()
    return B, H, W, feats, stab, un


@functools.lru_cache(maxsize=None)
def _noprev_pair():
    """Trainer() and the same trainer with objective=OBJECTIVE_NOPREV on one forward: (loss, parameter gradients, flow gradients) each."""
    B, H, W, feats, stab, un = _trainer_inputs(3)
    w = wts.synthetic_weights(seed=12, cin=27, random_bn=True, flow_gain=0.5)
    tr = train_step.Trainer(w, B, H, W)
    tr.forward(feats)
    out = []
    for objective, target in ((None, stab[..., :3].contiguous()), (training.OBJECTIVE_NOPREV, stab)):
        tr.objective = objective
        loss = tr.loss_and_backward(target, un)
        out.append((float(loss), tr.export(tr.g), {k: v.clone() for k, v in tr.dpf.items()}))
    return out


def test_trainer_noprev_objective_is_the_default_path_bit_for_bit():
    """One target of weight 1 inside vstab_loss_main_multi resizes the target's three channels alone and runs the T = 1 kernels
    vstab_loss_main runs, so gradients and loss value are the default path's.
    Level 2 is 94 x 126 here: three workgroups per sample in pass 1, whose fp64 atomics arrive in no fixed order, so the VALUE comparison
    below can miss by one ulp from run to run although both sides run the same kernels (measured on an MI355X, before and after the
    one-target kernels were merged into the T = 1 instance alike: 40 vstab_loss_level calls on this level gave two bit patterns of the
    sums, 38 : 2; six fused / multi pairs gave 0x1.89360af1a52c7p-1 on one side and ...c8p-1 on the other three times).  Up to two
    workgroups per sample (8192 pixels) the sum is order-independent.  The gradients read den rounded to float32 and do not see it."""
    a, b = _noprev_pair()
    assert a[0] == b[0], (a[0], b[0])
    for k in LEVELS:
        assert torch.equal(a[2][k], b[2][k]), k
    assert set(a[1]) == set(b[1])
    for k, v in a[1].items():
        assert np.array_equal(v, b[1][k]), k
    assert max(float(np.abs(v).max()) for v in a[1].values()) > 0


def test_one_target_objectives_through_loss_main_multi():
    """One target of weight 1 at any channel offset is loss_main_fused on that slice bit for bit (value, gradients, strided pixels);
    one target of another weight goes through the multi kernels and agrees within the reference bounds' scale."""
    stab, un, flows, _p = _case(0)
    s, u = stab.cuda(), un.cuda()
    wide = {k: torch.zeros(*v.shape[:3], 4).cuda() for k, v in flows.items()}
    for k, v in flows.items():
        wide[k][..., :2] = v.cuda()
    for c in (0, 9, 21):
        obj = training.Objective((c,), (1.0,), training.TV_WEIGHTS)
        g0 = {k: torch.full_like(v, 7.0) for k, v in wide.items()}
        g1 = {k: torch.full_like(v, 7.0) for k, v in wide.items()}
        l0 = training.loss_main_fused(wide, s[..., c:c + 3].contiguous(), u, g0)
        l1, per = training.loss_main_multi(wide, s, u, obj, g1)
        assert float(l0) == float(l1), c
        assert all(torch.equal(g0[k], g1[k]) for k in LEVELS), c
        tv = sum(w * float(vo.total_variation(flows[k])) for w, k in zip(training.TV_WEIGHTS, LEVELS))
        assert abs(float(per[0]) + tv - float(l1)) <= 1e-9
        # a 3-channel target tensor is the same call
        l3, _ = training.loss_main_multi(wide, s[..., c:c + 3].contiguous(), u, training.Objective((0,), (1.0,), training.TV_WEIGHTS))
        assert float(l3) == float(l1)
        half = training.Objective((c,), (0.5,), training.TV_WEIGHTS)
        gh = {k: torch.full_like(v, 7.0) for k, v in wide.items()}
        lh, perh = training.loss_main_multi(wide, s, u, half, gh)
        assert abs(float(perh[0]) - float(per[0])) <= 1e-12 * max(1.0, abs(float(per[0])))
        assert abs(float(lh) - (0.5 * float(per[0]) + tv)) <= 1e-9


def test_trainer_prev_objective_flow_gradients_and_descent():
    B, H, W, feats, stab, un = _trainer_inputs(1)
    w = wts.synthetic_weights(seed=5, cin=27, random_bn=False, flow_gain=0.2)
    obj = training.OBJECTIVE_PREV
    tr = train_step.Trainer(w, B, H, W, objective=obj)
    tr.forward(feats)
    backward = tr._backward
    tr._backward = lambda: None                    # look at dpf as the loss leaves it, before the network's backward accumulates into it
    try:
        loss = tr.loss_and_backward(stab, un)
    finally:
        tr._backward = backward
    grads = {k: torch.full_like(v, 7.0) for k, v in tr.pf.items()}
    want, _per = training.loss_main_multi(tr.pf, stab, un, obj, grads)
    assert float(loss) == float(want)
    for k in LEVELS:
        assert torch.equal(tr.dpf[k][..., :2], grads[k][..., :2]), k
        assert float(tr.dpf[k][..., 2:].abs().max()) == 0.0
    ref_loss, _rper, _g = ref.loss_and_gradients({k: v[..., :2].float().cpu() for k, v in tr.pf.items()}, stab.cpu(), un.cpu(), obj)
    assert abs(float(loss) - ref_loss) <= 2e-5 * max(1.0, abs(ref_loss))
    # three optimiser steps on the fixed batch lower the objective
    first = float(tr.step(feats, stab, un, lr=1e-4))
    for _ in range(2):
        tr.step(feats, stab, un, lr=1e-4)
    tr.forward(feats)
    after, _ = training.loss_main_multi(tr.pf, stab, un, obj)
    print(f"objective before {first:.6f} after three steps {float(after):.6f}")
    assert np.isfinite(first) and float(after) < first
    assert tr.train_epoch([(feats, stab, un)], epoch=0)[0] == pytest.approx(float(after), rel=1e-12)


# ----------------------------------------------------------------------------- 7. scale_mse, argument checks
def test_scale_mse_scales_the_photometric_gradient_only():
    """vstab_loss_level's scale_mse enters the gradient as k = scale_mse * 2 M^2 / (B den) and nothing else: the sums do not see it, and
    with scale_tv = 0 a power of two scales every gradient element exactly."""
    stab, un, flows, _p = _case(1)
    pf = flows["predict_flow3"].cuda()
    B, h, w, _ = pf.shape
    assert (B, h, w) == (1, 6, 8)
    G, U = resize_images(stab[..., :3].contiguous().cuda(), (h, w)), resize_images(un.cuda(), (h, w))
    got = {}
    for scale in (0.5, 1.0):
        sums, grad = torch.full((3 * B,), -1.0, dtype=torch.float64, device="cuda"), torch.full_like(pf, 7.0)
        _lib.check(_lib.lib().vstab_loss_level(pf.data_ptr(), G.data_ptr(), U.data_ptr(), B, h, w, sums.data_ptr(), scale, 0.0, grad.data_ptr(),
                                               runtime.stream_ptr()))
        got[scale] = (sums, grad)
    assert torch.equal(got[0.5][0], got[1.0][0])
    assert float(got[1.0][1].abs().max()) > 0.0
    assert torch.equal(2 * got[0.5][1], got[1.0][1])


def test_one_target_entry_points_have_the_limits_of_the_multi_target_ones():
    """B <= 65535 (gridDim.y) and h * w * 3 < 2^31 (32-bit tap offsets): VSTAB_E_SHAPE / a workspace size of 0 before anything is
    launched -- the buffers here are a few floats."""
    L = _lib.lib()
    SHAPE = -1
    small = torch.zeros(64).cuda()
    sums = torch.zeros(8, dtype=torch.float64).cuda()
    st = runtime.stream_ptr()

    def level(B, h, w):
        return L.vstab_loss_level(small.data_ptr(), small.data_ptr(), small.data_ptr(), B, h, w, sums.data_ptr(), 1.0, 0.0, None, st)

    assert level(1, 1, 2) == 0
    assert level(1, 1, 715827883) == SHAPE and b"loss_level" in L.vstab_last_error(None)            # h * w * 3 = 2^31 + 1
    assert level(65536, 1, 1) == SHAPE

    def main_bytes(B, h, w):
        d = (_lib.LossLevelDesc * 1)()
        d[0].pf, d[0].h, d[0].w, d[0].cs_pf, d[0].tv_weight = small.data_ptr(), h, w, 2, 0.0
        return d, L.vstab_loss_main_workspace_bytes(C.addressof(d), 1, B)

    assert main_bytes(1, 1, 715827883)[1] == 0 and main_bytes(65536, 1, 1)[1] == 0
    assert main_bytes(1, 1, 715827882)[1] > 2 * 4 * (2 ** 31 - 2)                                   # h * w * 3 = 2^31 - 2: sized, not launched
    d, n = main_bytes(1, 1, 2)
    out, ws = torch.zeros((), dtype=torch.float64).cuda(), torch.zeros(n, dtype=torch.uint8).cuda()
    big, _n = main_bytes(1, 1, 715827883)
    for desc, B in ((big, 1), (d, 65536)):
        assert L.vstab_loss_main(C.addressof(desc), 1, small.data_ptr(), small.data_ptr(), B, 1, 2, out.data_ptr(), ws.data_ptr(), n, st) == SHAPE
        assert b"loss_main" in L.vstab_last_error(None)
    assert L.vstab_loss_main(C.addressof(d), 1, small.data_ptr(), small.data_ptr(), 1, 1, 2, out.data_ptr(), ws.data_ptr(), n, st) == 0
    torch.cuda.synchronize()


def test_argument_checks():
    L = _lib.lib()
    B, h, w, Ct = 2, 5, 6, 24
    pf, G, U = torch.zeros(B, h, w, 2).cuda(), torch.zeros(B, h, w, Ct).cuda(), torch.zeros(B, h, w, 3).cuda()
    sums, grad = torch.zeros(10 * B, dtype=torch.float64).cuda(), torch.zeros(B, h, w, 2).cuda()
    st = runtime.stream_ptr()
    OK, SHAPE, ALIGN, NOMEM, STATE = 0, -1, -2, -4, -6

    def level(pf_=pf.data_ptr(), G_=G.data_ptr(), U_=U.data_ptr(), sums_=sums.data_ptr(), grad_=grad.data_ptr(), Ct_=Ct, offs=(0, 3), wts_=(1.0, 0.5),
              T=None, null_arrays=False):
        T = len(offs) if T is None else T
        n = max(len(offs), 1)
        a, b = (C.c_int32 * n)(*offs), (C.c_float * n)(*(tuple(wts_) + (0.0,) * n)[:n])
        rc = L.vstab_loss_level_multi(pf_, G_, Ct_, T, None if null_arrays else a, None if null_arrays else b, U_, B, h, w, sums_, 0.0, grad_, st)
        if rc != OK:
            assert b"loss_level_multi" in L.vstab_last_error(None)
        return rc

    assert level() == OK and level(grad_=None) == OK
    assert level(pf_=None) == STATE and level(G_=None) == STATE and level(U_=None) == STATE and level(sums_=None) == STATE
    assert level(null_arrays=True) == STATE
    assert level(T=0) == SHAPE and level(offs=tuple(range(0, 27, 3))[:9], wts_=(1.0,) * 9, Ct_=27) == SHAPE
    assert level(offs=tuple(range(0, 24, 3)), wts_=(1.0,) * 8) == OK                                  # T = 8 is the most
    assert level(offs=(0, 22)) == SHAPE and level(offs=(21,)) == OK and level(offs=(-1,)) == SHAPE    # c_off[t] + 3 > Ct
    assert level(offs=(0,), Ct_=2) == SHAPE
    assert level(pf_=pf.data_ptr() + 4) == ALIGN and level(grad_=grad.data_ptr() + 4) == ALIGN and level(sums_=sums.data_ptr() + 4) == ALIGN

    H, W = 10, 12
    stab, un = torch.zeros(B, H, W, Ct).cuda(), torch.zeros(B, H, W, 3).cuda()
    fl = {k: torch.zeros(B, h, w, 4).cuda() for k in LEVELS}
    gr = {k: torch.zeros(B, h, w, 4).cuda() for k in LEVELS}
    out = torch.zeros(9, dtype=torch.float64).cuda()

    def descs(cs_pf=4, cs_grad=4, pf_shift=0, grad_shift=0):
        d = (_lib.LossLevelDesc * 5)()
        for e, k in zip(d, LEVELS):
            e.pf, e.grad, e.h, e.w, e.cs_pf, e.cs_grad, e.tv_weight = fl[k].data_ptr() + pf_shift, gr[k].data_ptr() + grad_shift, h, w, cs_pf, cs_grad, 0.0
        return d

    good = descs()
    n = L.vstab_loss_main_multi_workspace_bytes(C.addressof(good), 5, B, Ct, 2)
    assert n >= 5 * 4 * B * 8 + B * h * w * (Ct + 3) * 4
    ws = torch.zeros(n + 8, dtype=torch.uint8).cuda()

    def main(d=good, n_levels=5, stab_=stab.data_ptr(), un_=un.data_ptr(), out_=out.data_ptr(), ws_=ws.data_ptr(), nbytes=n, Ct_=Ct, offs=(0, 3),
             T=None, null_arrays=False):
        T = len(offs) if T is None else T
        m = max(len(offs), 1)
        a, b = (C.c_int32 * m)(*offs), (C.c_float * m)(*([1.0] * m))
        rc = L.vstab_loss_main_multi(C.addressof(d), n_levels, stab_, Ct_, T, None if null_arrays else a, None if null_arrays else b, un_, B, H, W,
                                     out_, ws_, nbytes, st)
        if rc != OK:
            assert b"loss_main_multi" in L.vstab_last_error(None)
        return rc

    assert main() == OK
    assert main(stab_=None) == STATE and main(un_=None) == STATE and main(out_=None) == STATE and main(ws_=None) == STATE
    assert main(null_arrays=True) == STATE
    assert main(T=0) == SHAPE and main(offs=tuple(range(0, 27, 3)), Ct_=27) == SHAPE and main(n_levels=0) == SHAPE and main(n_levels=9) == SHAPE
    assert main(offs=(0, 22)) == SHAPE and main(offs=(-3,)) == SHAPE
    assert main(d=descs(cs_pf=3)) == SHAPE and main(d=descs(cs_grad=3)) == SHAPE                        # odd channel strides
    assert main(d=descs(pf_shift=4)) == ALIGN and main(d=descs(grad_shift=4)) == ALIGN
    assert main(out_=out.data_ptr() + 4) == ALIGN and main(ws_=ws.data_ptr() + 4) == ALIGN
    assert main(nbytes=n - 1) == NOMEM
    for bad in (descs(cs_pf=3), descs(pf_shift=4)):
        assert L.vstab_loss_main_multi_workspace_bytes(C.addressof(bad), 5, B, Ct, 2) == 0
    assert L.vstab_loss_main_multi_workspace_bytes(C.addressof(good), 5, B, Ct, 9) == 0
    torch.cuda.synchronize()

    # the Python wrappers turn every one of these into ValueError
    obj = training.Objective((0, 3), (1.0, 0.5), (0.0,) * 5)
    fl2 = {k: v[..., :2].contiguous() for k, v in fl.items()}
    training.loss_main_multi(fl2, stab, un, obj)
    training.lossterm_multi(pf, stab, un, (0, 3), (1.0, 0.5))
    for call in (lambda: training.lossterm_multi(pf, None, un, (0,), (1.0,)),
                 lambda: training.lossterm_multi(pf, stab, None, (0,), (1.0,)),
                 lambda: training.lossterm_multi(None, stab, un, (0,), (1.0,)),
                 lambda: training.lossterm_multi(pf, stab, un, (), ()),
                 lambda: training.lossterm_multi(pf, stab, un, tuple(range(0, 27, 3)), (1.0,) * 9),
                 lambda: training.lossterm_multi(pf, stab, un, (0, 3), (1.0,)),
                 lambda: training.lossterm_multi(pf, stab, un, (22,), (1.0,)),
                 lambda: training.lossterm_multi(pf, stab[..., :2].contiguous(), un, (0,), (1.0,)),
                 lambda: training.lossterm_multi(torch.zeros(B * h * w * 2 + 2).cuda()[1:-1].view(B, h, w, 2), stab, un, (0,), (1.0,)),
                 lambda: training.loss_main_multi(fl2, None, un, obj),
                 lambda: training.loss_main_multi(fl2, stab, un[:1], obj),
                 lambda: training.loss_main_multi(fl2, stab[..., :5].contiguous(), un, obj),
                 lambda: training.loss_main_multi({k: v[..., :3].contiguous() for k, v in fl.items()}, stab, un, obj),
                 lambda: training.loss_main_multi(fl2, stab, un, obj, {k: torch.zeros(B, h, w, 3).cuda() for k in LEVELS}),
                 lambda: training.loss_main_multi({k: torch.zeros(B * h * w * 2 + 2).cuda()[1:-1].view(B, h, w, 2) for k in LEVELS}, stab, un, obj)):
        with pytest.raises(ValueError):
            call()
