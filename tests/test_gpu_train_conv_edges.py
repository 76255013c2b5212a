"""The training step's three convolution entry points (`vstab_conv_forward`, `vstab_conv_dgrad`, `vstab_conv_wgrad`) on the paths the
Trainer takes and tests/test_gpu_training.py / test_gpu_kloop.py do not: one more output row / column than the symmetric-pad size
(A), the one-launch-per-phase plan of odd-k stride-2 input gradients next to the merged launch (B), channel slices on both sides,
every epilogue and every bias route of the forward, the dword-gather variant and its refusal (C), the transposed conv's bias (D).
References: tests/train_conv_ref.py (float64 on the CPU, pinned by tests/test_train_conv_ref_cpu.py).  Bound: 2e-5 max|ref| + 1e-6
as in test_gpu_training.py, 4e-5 for a second accumulating call.  Every buffer wider than its slice starts as random numbers and its
other channels must come back bit for bit.  Each comparison prints its error as a fraction of its bound (pytest -s)."""
import functools

import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime, training
from tests import train_conv_ref as ref

pytestmark = pytest.mark.gpu

E_SHAPE = -1


def _close(group, got, want, factor=2e-5, scale=None):
    got = got.double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    err = float((got - want).abs().max())
    tol = factor * (float(want.abs().max()) if scale is None else scale) + 1e-6
    print(f"[conv-edges {group}] err/tol {err / tol:.4f}")
    assert err <= tol, (group, err, tol)              # (a NaN fails too)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _forward(x, W, b, k, s, p, out_hw, cx_off=0, y=None, cy_off=0, act=0):
    """vstab_conv_forward on channels cx_off..+W.shape[2] of x into channels cy_off..+W.shape[3] of y (allocated when None).
    Returns (code, y, workspace bytes asked for)."""
    B, Hi, Wi, cs_x = x.shape
    cin, cout = W.shape[2], W.shape[3]
    Ho, Wo = out_hw
    if y is None:
        y = torch.empty(B, Ho, Wo, cout, dtype=torch.float32, device=x.device)
    assert y.shape[:3] == (B, Ho, Wo) and y.is_contiguous() and x.is_contiguous() and W.is_contiguous()
    cs_y = y.shape[3]
    L = _lib.lib()
    n = int(L.vstab_conv_forward_workspace_bytes(B, Hi, Wi, cs_x, cin, k, s, p, cout, cs_y, cy_off, act, Ho, Wo))
    ws = torch.empty(n + 256, dtype=torch.uint8, device=x.device)
    code = L.vstab_conv_forward(x.data_ptr(), B, Hi, Wi, cs_x, cx_off, cin, W.data_ptr(), b.data_ptr() if b is not None else None, k, s, p,
                                y.data_ptr(), Ho, Wo, cs_y, cy_off, cout, act, ws.data_ptr(), ws.numel(), runtime.stream_ptr())
    torch.cuda.synchronize()
    return code, y, n


def _forward_ok(*a, **kw):
    code, y, n = _forward(*a, **kw)
    _lib.check(code)
    assert n > 0
    return y


# ============================================================================= A. one more output row / column
_A = [pytest.param(c, d, id=f"{c[1]}x{c[2]}-{c[3]}to{c[4]}-k{c[5]}-+{d[0]}+{d[1]}") for c in ref.EXTRA_CASES for d in ref.EXTRA_DELTAS]


@pytest.mark.parametrize("case,delta", _A)
def test_forward_with_an_extra_row_or_column(case, delta):
    B, Hi, Wi, cin, cout, k, s, p = case
    hw = ref.extra_out_hw(case, delta)
    x, W, b, y0 = ref.rand_case(11, B, Hi, Wi, cin, cout, k, hw)
    y = _forward_ok(x.cuda(), W.cuda(), b.cuda(), k, s, p, hw)
    _close("A forward", y, ref.conv_ref(x, W, b, k, s, p, hw))
    ya = _forward_ok(x.cuda(), W.cuda(), None, k, s, p, hw, y=y0.cuda(), act=3)
    _close("A forward act3", ya, y0.double() + ref.conv_ref(x, W, None, k, s, p, hw))


@pytest.mark.parametrize("case,delta", _A)
def test_dgrad_with_an_extra_row_or_column(case, delta):
    B, Hi, Wi, cin, cout, k, s, p = case
    hw = ref.extra_out_hw(case, delta)
    _, W, _, _ = ref.rand_case(12, B, Hi, Wi, cin, cout, k, hw)
    gw = _randn(13, B, hw[0], hw[1], cout + 12)                   # the gradient lives in channels 8..8+cout
    g = gw[..., 8:8 + cout].contiguous()
    want = ref.dgrad_ref(g, W, None, k, s, p, (Hi, Wi))
    _close("A dgrad", training.conv_dgrad(g.cuda(), W.cuda(), s, p, (Hi, Wi)), want)
    base = _randn(14, B, Hi, Wi, cin + 8)                         # accumulate into channels 4..4+cin
    out = training.conv_dgrad(gw.cuda(), W.cuda(), s, p, (Hi, Wi), cg_off=8, cout=cout, dx=base.cuda(), cx_off=4, accumulate=True).cpu()
    total = base.double().clone()
    total[..., 4:4 + cin] += want
    _close("A dgrad accumulate", out, total)
    assert torch.equal(out[..., :4], base[..., :4]) and torch.equal(out[..., 4 + cin:], base[..., 4 + cin:])
    if (k, s, p) == (4, 2, 1):
        # the same call is DeConv2dLayer's forward (filter [4,4,out,in] = W) cropped to Hi x Wi, with its bias
        bias = _randn(15, cin)
        y = training.conv_dgrad(g.cuda(), W.cuda(), 2, 1, (Hi, Wi), bias=bias.cuda())
        _close("A deconv forward + bias", y, ref.deconv_ref(g, W, bias, (Hi, Wi)))


@pytest.mark.parametrize("case,delta", _A)
def test_wgrad_with_an_extra_row_or_column(case, delta):
    B, Hi, Wi, cin, cout, k, s, p = case
    hw = ref.extra_out_hw(case, delta)
    x, _, _, g = ref.rand_case(16, B, Hi, Wi, cin, cout, k, hw)
    rW, rb = ref.wgrad_ref(x, g, k, s, p)
    dW, db = training.conv_wgrad(x.cuda(), g.cuda(), k, s, p)
    _close("A wgrad dW", dW, rW)
    _close("A wgrad db", db, rb)
    dW2, db2 = training.conv_wgrad(x.cuda(), g.cuda(), k, s, p, dW=dW.clone(), db=db.clone(), accumulate=True)
    _close("A wgrad dW twice", dW2, 2 * rW, factor=4e-5, scale=float(rW.abs().max()))
    _close("A wgrad db twice", db2, 2 * rb, factor=4e-5, scale=float(rb.abs().max()))
    if (k, s, p) == (4, 2, 1):
        # (input, gout) = (dy, x) of a cropped DeConv2dLayer: its [4,4,out,in] filter gradient, from torch's transposed conv
        import torch.nn.functional as F
        Wt = torch.zeros(cout, cin, 4, 4, dtype=torch.float64, requires_grad=True)
        yt = F.conv_transpose2d(g.double().permute(0, 3, 1, 2), Wt, stride=2, padding=1, output_padding=1)[:, :, :Hi, :Wi]
        yt.backward(x.double().permute(0, 3, 1, 2))
        _close("A deconv filter gradient", dW, Wt.grad.permute(2, 3, 1, 0).contiguous())


def test_sizes_beyond_one_extra_row_are_refused():
    """stride 1 takes no extra row in the input gradient; nobody takes two.  Refused before anything is written."""
    dx0 = _randn(17, 1, 9, 11, 8)
    W1 = _randn(18, 3, 3, 8, 8).cuda()
    for ghw in ((10, 11), (9, 12), (10, 12)):
        dx = dx0.cuda()
        with pytest.raises(ValueError):
            training.conv_dgrad(torch.zeros(1, ghw[0], ghw[1], 8).cuda(), W1, 1, 1, (9, 11), dx=dx, accumulate=True)
        torch.cuda.synchronize()
        assert torch.equal(dx.cpu(), dx0)
    B, Hi, Wi, cin, cout, k, s, p = ref.EXTRA_CASES[0]
    for d in ((2, 0), (0, 2), (2, 2), (-1, 0)):
        hw = ref.extra_out_hw(ref.EXTRA_CASES[0], d)
        x, W, b, g = ref.rand_case(19, B, Hi, Wi, cin, cout, k, hw)
        with pytest.raises(ValueError):
            training.conv_wgrad(x.cuda(), g.cuda(), k, s, p)
        dx0 = _randn(20, B, Hi, Wi, cin)
        dx = dx0.cuda()
        with pytest.raises(ValueError):
            training.conv_dgrad(g.cuda(), W.cuda(), s, p, (Hi, Wi), dx=dx, accumulate=True)
        y0 = _randn(21, *g.shape)
        code, y, n = _forward(x.cuda(), W.cuda(), b.cuda(), k, s, p, hw, y=y0.cuda())
        assert code == E_SHAPE and n == 0
        assert torch.equal(y.cpu(), y0) and torch.equal(dx.cpu(), dx0)


# ============================================================================= B. merged launch / one launch per phase
@functools.lru_cache(maxsize=None)
def _phase_case(i):
    """(wide gout, its slice, W, the float64 input gradient) of PHASE_CASES[i], computed once for the plain and the accumulating test"""
    case = ref.PHASE_CASES[i]
    B, Hi, Wi, cin, cout, k, p = case[:7]
    hw = ref.phase_out_hw(case)
    gen = torch.Generator().manual_seed(100 + i)
    gw = torch.randn(B, hw[0], hw[1], cout + 8, generator=gen)              # gradient in channels 4..4+cout
    W = torch.randn(k, k, cin, cout, generator=gen) / (k * k * cin) ** 0.5
    g = gw[..., 4:4 + cout].contiguous()
    return gw, g, W, ref.dgrad_ref(g, W, None, k, 2, p, (Hi, Wi))


_B = [pytest.param(i, id=f"{c[0]}x{c[1]}x{c[2]}-{c[3]}from{c[4]}-k{c[5]}-{'extra-' if c[7] else ''}{'per-phase' if c[9] else 'merged'}")
      for i, c in enumerate(ref.PHASE_CASES)]


@pytest.mark.parametrize("i", _B)
def test_odd_k_stride2_dgrad_on_both_plans(i):
    B, Hi, Wi, cin, cout, k, p = ref.PHASE_CASES[i][:7]
    assert (ref.dgrad_plan_tiles(B, Hi, Wi, cin, k, p) > ref.PHASE_THRESHOLD) == ref.PHASE_CASES[i][9]
    _, g, W, want = _phase_case(i)
    _close("B dgrad", training.conv_dgrad(g.cuda(), W.cuda(), 2, p, (Hi, Wi)), want)


@pytest.mark.parametrize("i", _B)
def test_odd_k_stride2_dgrad_on_both_plans_accumulating_into_a_slice(i):
    """act = 3 once per launch on disjoint parity pixels, the gradient read at cg_off = 4, the result added to channels 4..4+cin"""
    B, Hi, Wi, cin, cout, k, p = ref.PHASE_CASES[i][:7]
    gw, _, W, want = _phase_case(i)
    base = _randn(200 + i, B, Hi, Wi, cin + 8)
    out = training.conv_dgrad(gw.cuda(), W.cuda(), 2, p, (Hi, Wi), cg_off=4, cout=cout, dx=base.cuda(), cx_off=4, accumulate=True).cpu()
    total = base.double().clone()
    total[..., 4:4 + cin] += want
    _close("B dgrad accumulate", out, total)
    assert torch.equal(out[..., :4], base[..., :4]) and torch.equal(out[..., 4 + cin:], base[..., 4 + cin:])


# ============================================================================= C. vstab_conv_forward: slices, epilogues, bias routes
CB, CH, CW = 2, 9, 11                   # base shape: 3x3, stride 1, pad 1


@pytest.mark.parametrize("cin,cs_x,cx_off,cout", [(8, 20, 4, 24),       # a run of 72 floats against nine 8-float taps
                                                  (32, 40, 4, 64)])     # the blocked [K][N] operand against the gather table
def test_forward_input_slice_equals_the_contiguous_call(cin, cs_x, cx_off, cout):
    xw = _randn(30 + cin, CB, CH, CW, cs_x)
    _, W, b, _ = ref.rand_case(31, CB, CH, CW, cin, cout, 3, (CH, CW))
    xs = xw[..., cx_off:cx_off + cin].contiguous()
    want = ref.conv_ref(xs, W, b, 3, 1, 1, (CH, CW))
    y_slice = _forward_ok(xw.cuda(), W.cuda(), b.cuda(), 3, 1, 1, (CH, CW), cx_off=cx_off)
    y_cont = _forward_ok(xs.cuda(), W.cuda(), b.cuda(), 3, 1, 1, (CH, CW))
    _close("C input slice", y_slice, want)
    _close("C input slice (contiguous copy)", y_cont, want)
    assert float((y_slice - y_cont).abs().max()) <= 2e-6 * float(want.abs().max())


@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", [0, 1, 2, 3])
def test_forward_output_slice_every_epilogue(act, with_bias):
    """cout = 12 at cy_off = 8 of 28-wide pixels; act 3 adds to what the slice held"""
    cin, cout, cs_y, cy_off = 8, 12, 28, 8
    x, W, b, _ = ref.rand_case(40 + act, CB, CH, CW, cin, cout, 3, (CH, CW))
    y0 = _randn(41, CB, CH, CW, cs_y)
    want = ref.act_ref(ref.conv_ref(x, W, b if with_bias else None, 3, 1, 1, (CH, CW)), act, y0[..., cy_off:cy_off + cout])
    if act in (1, 2):
        assert float(want.min()) < -0.05 if act == 1 else float((want == 0).double().mean()) > 0.2        # the epilogue acts on these inputs
    y = _forward_ok(x.cuda(), W.cuda(), b.cuda() if with_bias else None, 3, 1, 1, (CH, CW), y=y0.cuda(), cy_off=cy_off, act=act).cpu()
    _close(f"C output slice act {act}", y[..., cy_off:cy_off + cout], want)
    assert torch.equal(y[..., :cy_off], y0[..., :cy_off]) and torch.equal(y[..., cy_off + cout:], y0[..., cy_off + cout:])


def test_forward_act3_with_bias_under_split_k():
    """a reduction of 144 K-tiles on a single 128-column tile is split; the bias and what y held are added once, not once per slab"""
    B, H, Wd, cin, cout = 1, 8, 8, 512, 128
    x, W, b, y0 = ref.rand_case(45, B, H, Wd, cin, cout, 3, (H, Wd))
    code, y, n = _forward(x.cuda(), W.cuda(), b.cuda(), 3, 1, 1, (H, Wd), y=y0.cuda(), act=3)
    _lib.check(code)
    packed = 9 * cin * cout * 4
    assert n > packed + 2 * B * H * Wd * cout * 4, "the plan no longer splits this reduction: choose a shape that does"
    _close("C act3 + bias, split-K", y, y0.double() + ref.conv_ref(x, W, b, 3, 1, 1, (H, Wd)))
    y1 = _forward_ok(x.cuda(), W.cuda(), b.cuda(), 3, 1, 1, (H, Wd), act=1)
    _close("C act1 + bias, split-K", y1, ref.act_ref(ref.conv_ref(x, W, b, 3, 1, 1, (H, Wd)), 1))


def test_forward_bias_routes():
    """no bias: the shared zero vector; cout == Npad (64, 128): the caller's pointer; cout = 60: a padded copy in the workspace.  One
    process, another bias each call, 60 after 64 and after 128: a stale padded copy or a stale pointer would show."""
    cin = 32
    x = _randn(50, CB, CH, CW, cin)
    xd = x.cuda()
    for n, cout in enumerate((64, 60, 128, 60, 64)):
        _, W, b, _ = ref.rand_case(51 + n, CB, CH, CW, cin, cout, 3, (CH, CW))
        b = b * 3.0
        for bias in (b, None):
            y = _forward_ok(xd, W.cuda(), bias.cuda() if bias is not None else None, 3, 1, 1, (CH, CW))
            _close(f"C bias route cout {cout}", y, ref.conv_ref(x, W, bias, 3, 1, 1, (CH, CW)))


@pytest.mark.parametrize("cout,cs_y", [(2, 4), (18, 20), (18, 18)], ids=["2in4", "18in20", "18in18"])
@pytest.mark.parametrize("act", [0, 1])
def test_forward_column_counts_that_are_no_multiple_of_4(cout, cs_y, act):
    """the 2-channel heads in 4-wide pixels: a last 16-byte group that is partly live (18 in 18: pixels that are not 16-byte
    friendly at all, the 4-byte epilogue).  No split-K for these."""
    cin = 8
    x, W, b, _ = ref.rand_case(60 + cout, CB, CH, CW, cin, cout, 3, (CH, CW))
    y0 = _randn(61, CB, CH, CW, cs_y)
    y = _forward_ok(x.cuda(), W.cuda(), b.cuda(), 3, 1, 1, (CH, CW), y=y0.cuda(), act=act).cpu()
    _close(f"C cout {cout} in {cs_y}", y[..., :cout], ref.act_ref(ref.conv_ref(x, W, b, 3, 1, 1, (CH, CW)), act))
    assert torch.equal(y[..., cout:], y0[..., cout:])


def test_forward_dword_gather_variant_and_its_refusal():
    """27 of 28 channels, 7x7 stride 2: taps of 27 floats cannot be read 16 bytes at a time.  The variant exists for the 128x64 tile
    (32 < cout < 128) only; other widths are refused before anything is written."""
    B, H, Wd, cin, cs_x = 2, 20, 24, 27, 28
    hw = (ref.min_out(H, 7, 2, 3), ref.min_out(Wd, 7, 2, 3))
    xw = _randn(70, B, H, Wd, cs_x)
    xs = xw[..., :cin].contiguous()
    for cout, taken in ((64, True), (24, False), (128, False)):
        _, W, b, _ = ref.rand_case(71 + cout, B, H, Wd, cin, cout, 7, hw)
        y0 = _randn(72, B, hw[0], hw[1], cout)
        code, y, n = _forward(xw.cuda(), W.cuda(), b.cuda(), 7, 2, 3, hw, y=y0.cuda())
        if taken:
            _lib.check(code)
            assert n > 0
            _close("C dword gather", y, ref.conv_ref(xs, W, b, 7, 2, 3, hw))
        else:
            assert code == E_SHAPE and n == 0
            assert torch.equal(y.cpu(), y0)


# ============================================================================= D. conv_dgrad with the transposed conv's bias
@pytest.mark.parametrize("cin", [64, 128, 16])
def test_dgrad_with_bias(cin):
    """DeConv2dLayer forward 8 -> cin of a 5x6 map cropped to 9x11: cin == Npad (64, 128) hands the caller's pointer to the kernel,
    16 goes through a padded copy; that one also accumulating into a slice"""
    B, Hi, Wi, cout, k, s, p = 2, 9, 11, 8, 4, 2, 1
    hw = (ref.min_out(Hi, k, s, p) + 1, ref.min_out(Wi, k, s, p) + 1)
    assert hw == (5, 6)
    _, W, _, g = ref.rand_case(80 + cin, B, Hi, Wi, cin, cout, k, hw)
    bias = _randn(81, cin) * 3.0
    want = ref.dgrad_ref(g, W, bias, k, s, p, (Hi, Wi))
    _close(f"D dgrad + bias cin {cin}", training.conv_dgrad(g.cuda(), W.cuda(), s, p, (Hi, Wi), bias=bias.cuda()), want)
    _close(f"D dgrad + bias cin {cin} (torch's transposed conv)", training.conv_dgrad(g.cuda(), W.cuda(), s, p, (Hi, Wi), bias=bias.cuda()),
           ref.deconv_ref(g, W, bias, (Hi, Wi)))
    _close(f"D dgrad no bias cin {cin}", training.conv_dgrad(g.cuda(), W.cuda(), s, p, (Hi, Wi)), ref.dgrad_ref(g, W, None, k, s, p, (Hi, Wi)))
    if cin == 16:
        base = _randn(82, B, Hi, Wi, cin + 8)
        out = training.conv_dgrad(g.cuda(), W.cuda(), s, p, (Hi, Wi), dx=base.cuda(), cx_off=4, accumulate=True, bias=bias.cuda()).cpu()
        total = base.double().clone()
        total[..., 4:4 + cin] += want
        _close("D dgrad + bias accumulate", out, total)
        assert torch.equal(out[..., :4], base[..., :4]) and torch.equal(out[..., 4 + cin:], base[..., 4 + cin:])
