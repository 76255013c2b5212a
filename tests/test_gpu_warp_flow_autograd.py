"""warp_flow.py under torch.autograd: every public function yields a grad_fn only when an input requires grad (and gradients are
enabled), returns the parent's bits otherwise, and its backward is the corresponding training.*_backward call -- bit-equal for the
atomic-free gradients (d flow, the resize and glue adjoints), within the d img bound of tests/test_gpu_warp_flow_backward.py for the
image gradients of the two gathers."""
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import training, utils, warp_flow
from tests import warp_flow_grad_ref as ref
from tests.test_gpu_warp_flow_backward import B, EPS, H, W, _b_img, _case, _check

pytestmark = pytest.mark.gpu
NET_H, NET_W, PH, PW = 24, 32, 22, 30                    # a network input of 24 x 32: predict_flow2 is 22 x 30


def _plain(fn, *args):
    """the call with nothing requiring grad, and under no_grad with everything requiring grad: no grad_fn, the same bits"""
    detached = [a.detach() if torch.is_tensor(a) else a for a in args]
    y = fn(*detached)
    with torch.no_grad():
        q = fn(*[a.detach().requires_grad_(True) if torch.is_tensor(a) and a.is_floating_point() else a for a in args])
    for t in (y, q):
        assert t.grad_fn is None and not t.requires_grad
    assert torch.equal(y, q)
    return y


@pytest.mark.parametrize("C_", [3, 4])
def test_tf_warp(C_):
    img, flow, dout, r, _ = _case("subpixel", C_)
    ic, fc, dc = img.cuda().requires_grad_(True), flow.cuda().requires_grad_(True), dout.cuda()
    y = warp_flow.tf_warp(ic, fc, H, W)
    assert y.grad_fn is not None
    g_img, g_flow = torch.autograd.grad(y, (ic, fc), dc)
    e_img, e_flow = training.warp_flow_backward(img.cuda(), flow.cuda(), dc)
    assert torch.equal(g_flow, e_flow)
    _check("autograd d_img", g_img, r["d_img"], _b_img(r))
    assert torch.equal(_plain(lambda i, f: warp_flow.tf_warp(i, f, H, W), ic, fc), y.detach())
    # one input frozen: only the other gradient is computed, and the flow's is the same sum
    (g2,) = torch.autograd.grad(warp_flow.tf_warp(img.cuda(), fc, H, W), (fc,), dc)
    assert torch.equal(g2, e_flow)
    y3 = warp_flow.tf_warp(ic, flow.cuda(), H, W)
    assert y3.grad_fn is not None
    _check("autograd d_img alone", torch.autograd.grad(y3, (ic,), dc)[0], r["d_img"], _b_img(r))


def test_get_pixel_value():
    g = torch.Generator().manual_seed(2)
    Hi, Wi, C_ = 11, 13, 3
    img = torch.rand(B, Hi, Wi, C_, generator=g).cuda().requires_grad_(True)
    x, y = torch.randint(-2, Wi + 2, (B, H, W), generator=g, dtype=torch.int32), torch.randint(-2, Hi + 2, (B, H, W), generator=g, dtype=torch.int32)
    dout = torch.randn(B, H, W, C_, generator=g)
    out = warp_flow.get_pixel_value(img, x, y)
    assert out.grad_fn is not None
    r = ref.get_pixel_value_backward(dout, x, y, Hi, Wi)
    _check("autograd get_pixel_value", torch.autograd.grad(out, (img,), dout.cuda())[0], r["d_img"], (r["n_img"] - 1).clamp_min(0) * EPS * r["S_img"])
    assert torch.equal(_plain(warp_flow.get_pixel_value, img, x, y), out.detach())


def test_resize_images_and_slice3():
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 9, 13, 5, generator=g).cuda().requires_grad_(True)
    dout = torch.randn(B, H, W, 5, generator=g).cuda()
    y = warp_flow.resize_images(x, (H, W))
    assert y.grad_fn is not None
    assert torch.equal(torch.autograd.grad(y, (x,), dout)[0], training.resize_bilinear_backward(dout, (9, 13)))
    assert torch.equal(_plain(lambda t: warp_flow.resize_images(t, (H, W)), x), y.detach())
    d3 = dout[..., :3].contiguous()
    z = warp_flow.resize_images_slice3(x, 1, (H, W))
    assert z.grad_fn is not None
    want = torch.zeros_like(x)
    want[..., 1:4] = training.resize_bilinear_backward(d3, (9, 13))
    assert torch.equal(torch.autograd.grad(z, (x,), d3)[0], want)
    assert torch.equal(_plain(lambda t: warp_flow.resize_images_slice3(t, 1, (H, W)), x), z.detach())
    assert torch.equal(z.detach(), warp_flow.resize_images(x.detach()[..., 1:4].contiguous(), (H, W)))


def test_flow_to_output_res():
    g = torch.Generator().manual_seed(4)
    pf = torch.randn(B, PH, PW, 2, generator=g).cuda().requires_grad_(True)
    dout = torch.randn(B, H, W, 2, generator=g).cuda()
    y = warp_flow.flow_to_output_res(pf, NET_H, NET_W, H, W)
    assert y.grad_fn is not None
    assert torch.equal(torch.autograd.grad(y, (pf,), dout)[0], training.flow_resize_scale_backward(dout, (PH, PW), NET_H, NET_W))
    assert torch.equal(_plain(lambda t: warp_flow.flow_to_output_res(t, NET_H, NET_W, H, W), pf), y.detach())


@pytest.mark.parametrize("want_outflow", [True, False])
def test_flow_glue_warp_is_the_chain_done_by_hand(want_outflow):
    g = torch.Generator().manual_seed(5)
    pf = (2.0 * torch.randn(B, PH, PW, 2, generator=g)).cuda()
    frame = torch.rand(B, H, W, 3, generator=g).cuda()
    d_warped = torch.randn(B, H, W, 3, generator=g).cuda()
    g_outflow = torch.randn(B, H, W, 2, generator=g).cuda()
    pfg, fg = pf.clone().requires_grad_(True), frame.clone().requires_grad_(True)
    outflow, warped = warp_flow.flow_glue_warp(pfg, fg, NET_H, NET_W, want_outflow)
    assert warped.grad_fn is not None and (outflow is None) == (not want_outflow)
    # today's call: no graph, the same bits, with nothing requiring grad and under no_grad
    p_of, p_w = warp_flow.flow_glue_warp(pf, frame, NET_H, NET_W, want_outflow)
    with torch.no_grad():
        q_of, q_w = warp_flow.flow_glue_warp(pfg, fg, NET_H, NET_W, want_outflow)
    for t in (p_w, q_w):
        assert t.grad_fn is None and torch.equal(t, warped.detach())
    if want_outflow:
        assert outflow.grad_fn is not None and p_of.grad_fn is None and q_of.grad_fn is None and torch.equal(p_of, outflow.detach()) and torch.equal(q_of, p_of)
    # by hand: the warp backward at output resolution, then the glue's adjoint
    of = warp_flow.flow_to_output_res(pf, NET_H, NET_W, H, W)
    e_img, e_of = training.warp_flow_backward(frame, of, d_warped)
    e_pf = training.flow_resize_scale_backward(e_of, (PH, PW), NET_H, NET_W)
    g_pf, g_frame = torch.autograd.grad(warped, (pfg, fg), d_warped, retain_graph=True)
    assert torch.equal(g_pf, e_pf)
    rr = ref.backward(*ref.warp(frame.cpu(), of.cpu()), d_warped.cpu())
    _check("glue autograd d_frame", g_frame, rr["d_img"], _b_img(rr))
    _check("glue explicit d_frame", e_img, rr["d_img"], _b_img(rr))
    if want_outflow:
        # a gradient arriving on outflow is added to the warp's before the glue's adjoint; outflow alone goes through the adjoint alone
        (g_pf2,) = torch.autograd.grad((warped, outflow), (pfg,), (d_warped, g_outflow), retain_graph=True)
        assert torch.equal(g_pf2, training.flow_resize_scale_backward(e_of + g_outflow, (PH, PW), NET_H, NET_W))
        (g_pf3,) = torch.autograd.grad(outflow, (pfg,), g_outflow)
        assert torch.equal(g_pf3, training.flow_resize_scale_backward(g_outflow, (PH, PW), NET_H, NET_W))
    # a frozen frame: the same d pf2
    w2 = warp_flow.flow_glue_warp(pfg, frame, NET_H, NET_W, want_outflow)[1]
    assert torch.equal(torch.autograd.grad(w2, (pfg,), d_warped)[0], e_pf)


def test_ssim_of_a_warped_frame_fills_flow_grad():
    """The motivating case: utils.tf_ssim(tf_warp(img, flow, H, W), target).backward() -- bit-equal to training.ssim_backward followed
    by training.warp_flow_backward."""
    img, flow, _, _, _ = _case("subpixel", 1)
    g = torch.Generator().manual_seed(6)
    target = (0.8 * img + 0.2 * torch.rand(img.shape, generator=g)).cuda()
    ic, fc = img.cuda(), flow.cuda().requires_grad_(True)
    utils.tf_ssim(warp_flow.tf_warp(ic, fc, H, W), target).backward()
    assert fc.grad is not None and bool(torch.isfinite(fc.grad).all()) and float(fc.grad.abs().max()) > 0
    warped = warp_flow.tf_warp(ic, flow.cuda(), H, W)
    d_warped, _ = training.ssim_backward(warped, target, torch.full((B,), 1.0 / B, device="cuda"), need_img2=False)
    assert torch.equal(fc.grad, training.warp_flow_backward(ic, flow.cuda(), d_warped, need_img=False)[1])
