"""The first layer on the bf16 MFMA (csrc/conv1_bf16x3.hip: fp32 operands split into three bf16 pieces, six piece-products per multiply,
fp32 accumulation) against the fp64 oracle and against the fp32 MFMA form (VSTAB_PLAN_CONV1_FP32 = plan flag 32).

The error bound is the issue's: max-abs error against fp64, in fp32 epsilons of max|y|, at most twice the fp32 form's on the same case.
Both forms run the same tiles over the same window, so the cases are the row-window kernel's: the minimum, ragged right and bottom
edges, more than one workgroup per row, an odd batch.  (2, 66, 70) is not a row-window geometry (70 * 27 floats per row is no multiple
of four): there both settings run the generic fp32 kernel and the bound holds trivially; (2, 66, 68) is the ragged case the new kernel
itself runs, and (1, 512, 384) the smallest launch that takes 128-pixel tiles (512 workgroups) with a 64-pixel tail launch."""
import numpy as np
import pytest
import torch

import coupe.optical_flow_based_deep_video_stabilization_amd as vs
from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime, weights as wts
from oracle import vstab_oracle as vo

pytestmark = pytest.mark.gpu
EPS = 1.1920929e-07
FLOW_TOL = 1e-3          # tests/test_gpu_parity.py
CONV1_FP32 = 32

SHAPES = [(1, 64, 64), (2, 66, 70), (1, 128, 256), (3, 64, 96), (2, 66, 68), (1, 512, 384)]
WEIGHTS = {"random_bn": lambda: wts.synthetic_weights(seed=11, cin=27, random_bn=True),
           "bench": lambda: wts.synthetic_weights(seed=1, cin=27)}
_ref_cache = {}


def dev(a):
    return torch.as_tensor(np.asarray(a)).to("cuda")


def case(wname, B, H, W):
    """weights, input and the oracle's fp64 conv1 (model.py:807-809), computed once per case"""
    key = (wname, B, H, W)
    if key not in _ref_cache:
        w = WEIGHTS[wname]()
        feats = np.random.default_rng(B * 1000 + H + W).random((B, H, W, 27), dtype=np.float32)
        t = {k: torch.from_numpy(w[f"1/{k}"]).double() for k in ("W_conv2d", "b_conv2d", "beta", "moving_mean", "moving_variance")}
        y = vo.pad_conv(torch.from_numpy(feats).double(), t["W_conv2d"], t["b_conv2d"], 3, 2)
        ref = vo.bn_lrelu(y, t["beta"], t["moving_mean"], t["moving_variance"])
        _ref_cache[key] = (w, feats, ref)
    return _ref_cache[key]


def context(w, flags):
    runtime.reset()
    vs.assign_weights(w)
    ctx = runtime.get_context()
    ctx.set_plan_flags(flags)
    return ctx


def conv1_of_forward(w, feats, flags):
    """conv1 as the forward leaves it in the workspace (the every-layer parity test's view), and the kernel that wrote it"""
    ctx = context(w, flags)
    try:
        ctx.profile(True)
        vs.flownetS_pyramid(dev(feats), feats.shape[0], is_train=False)
        torch.cuda.synchronize()
        name = ctx.profile_kernel_names()[0]
        ctx.profile(False)
        return ctx.internals(*feats.shape)["conv1"].clone().cpu(), name
    finally:
        ctx.set_plan_flags(0)


def conv1_alone(ctx, x, out, c_off=0):
    B, H, W, Cin = x.shape
    L = _lib.lib()
    _lib.check(L.vstab_conv1_forward(ctx._h, x.data_ptr(), B, H, W, Cin, out.data_ptr(), out.shape[3], c_off, runtime.stream_ptr()), ctx._h)
    torch.cuda.synchronize()


def err_eps(y, ref):
    return float((y.double() - ref).abs().max() / (EPS * ref.abs().max()))


@pytest.mark.parametrize("wname", list(WEIGHTS))
@pytest.mark.parametrize("B,H,W", SHAPES)
def test_error_within_twice_the_fp32_form(B, H, W, wname):
    w, feats, ref = case(wname, B, H, W)
    new, kn = conv1_of_forward(w, feats, 0)
    old, ko = conv1_of_forward(w, feats, CONV1_FP32)
    e_new, e_old = err_eps(new, ref), err_eps(old, ref)
    print(f"conv1 {B}x{H}x{W} {wname}: {kn} {e_new:.2f} eps of max|y|, {ko} {e_old:.2f}")
    assert "conv1_bf16x3" not in ko
    if (W * 27) % 4 == 0:
        assert kn.startswith("conv1_bf16x3_kernel") and ko.startswith("conv_rowwin_kernel")
    assert e_new <= 2.0 * e_old, (e_new, e_old)


def test_deterministic_and_the_same_bits_whatever_the_batch():
    w, feats, _ = case("random_bn", 3, 64, 96)
    ctx = context(w, 0)
    x = dev(feats)
    a, b, one = (torch.empty(n, 32, 48, 64, device="cuda") for n in (3, 3, 1))
    conv1_alone(ctx, x, a)
    conv1_alone(ctx, x, b)
    assert torch.equal(a, b)
    conv1_alone(ctx, x[1:2].contiguous(), one)       # the sums of a sample do not depend on what it is batched with
    assert torch.equal(one[0], a[1])


@pytest.mark.parametrize("B,H,W", [(1, 64, 64), (2, 66, 68), (1, 128, 256), (1, 512, 384)])
def test_concat_layout_untouched_channels_keep_the_sentinel(B, H, W):
    w, feats, ref = case("random_bn", B, H, W)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    for flags in (0, CONV1_FP32):
        ctx = context(w, flags)
        try:
            out = torch.full((B, Ho, Wo, 76), -777.0, device="cuda")
            conv1_alone(ctx, dev(feats), out, c_off=8)
            assert bool((out[..., :8] == -777.0).all()) and bool((out[..., 72:] == -777.0).all())
            got = out[..., 8:72].cpu()
            if flags == 0:
                plain = torch.empty(B, Ho, Wo, 64, device="cuda")
                conv1_alone(ctx, dev(feats), plain)
                assert torch.equal(plain.cpu(), got)          # the slice holds what the plain buffer holds
            assert err_eps(got, ref) <= 64.0
        finally:
            ctx.set_plan_flags(0)


def test_inf_and_nan_propagate_like_the_fp32_form():
    w, feats, _ = case("random_bn", 1, 64, 64)
    feats = feats.copy()
    feats[0, 10, 20, 5] = np.nan
    feats[0, 40, 41, 13] = np.inf
    feats[0, 63, 0, 26] = -np.inf
    outs = {}
    for flags in (0, CONV1_FP32):
        ctx = context(w, flags)
        try:
            out = torch.empty(1, 32, 32, 64, device="cuda")
            conv1_alone(ctx, dev(feats), out)
            outs[flags] = out.cpu()
        finally:
            ctx.set_plan_flags(0)
    new, old = outs[0], outs[CONV1_FP32]
    field = torch.zeros(32, 32, dtype=torch.bool)         # output pixels whose 7x7 stride-2 pad-3 field holds a marked input
    for (y, x) in [(10, 20), (40, 41), (63, 0)]:
        for oy in range(32):
            for ox in range(32):
                if 0 <= y - 2 * oy + 3 <= 6 and 0 <= x - 2 * ox + 3 <= 6:
                    field[oy, ox] = True
    nan_field = torch.zeros(32, 32, dtype=torch.bool)
    for oy in range(32):
        for ox in range(32):
            if 0 <= 10 - 2 * oy + 3 <= 6 and 0 <= 20 - 2 * ox + 3 <= 6:
                nan_field[oy, ox] = True
    assert not torch.isfinite(old[0][field]).any() and not torch.isfinite(new[0][field]).any()      # never finite garbage
    assert torch.isnan(old[0][nan_field]).all() and torch.isnan(new[0][nan_field]).all()            # NaN in, NaN out
    assert torch.isnan(new[0][field]).all()               # an infinity's middle piece is inf - inf: NaN where the fp32 form has +-inf or NaN
    # pixels that read none of the marked inputs through a live weight are finite in both forms, and agree
    clean = torch.isfinite(old[0]).all(dim=2) & torch.isfinite(new[0]).all(dim=2)
    assert int(clean.sum()) >= 32 * 32 - int(field.sum()) - 3 * 32
    assert float((new[0][clean] - old[0][clean]).abs().max()) <= 64 * EPS * float(old[0][clean].abs().max())


def test_whole_network_flows_within_flow_tol():
    w = wts.synthetic_weights(seed=9, cin=27, random_bn=True, flow_gain=2.0)
    feats = np.random.default_rng(9).random((1, 64, 80, 27), dtype=np.float32)
    ref = vo.flownetS_pyramid(feats, w, torch.float64)
    ctx = context(w, 0)
    ctx.profile(True)
    out = vs.flownetS_pyramid(dev(feats), 1, is_train=False)
    torch.cuda.synchronize()
    assert ctx.profile_kernel_names()[0].startswith("conv1_bf16x3_kernel")
    ctx.profile(False)
    errs = {k: float((out[k].double().cpu() - ref[k].double()).abs().max()) for k in vo.FLOW_KEYS}
    assert all(e <= FLOW_TOL for e in errs.values()), errs
    assert float(ref["predict_flow2"].abs().max()) > 0.5
