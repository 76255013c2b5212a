"""Pins tests/train_conv_ref.py on the CPU, in float64: the three references are each other's adjoints, the cropped
conv_transpose2d is the input gradient, every extra output row / column of the shared case tables reads the image (a case whose
extra row sees padding only proves nothing), and every phase-plan case lies on its side of dgrad_plan's 256-tile threshold."""
import pytest
import torch

from tests import train_conv_ref as ref


def _dot(a, b):
    return float((a.double() * b.double()).sum())


def _rel(a, b):
    return abs(a - b) / max(abs(a), abs(b))


def _adjoint_identities(x, W, g, k, s, p, out_hw):
    y = ref.conv_ref(x, W, None, k, s, p, out_hw)
    dx = ref.dgrad_ref(g, W, None, k, s, p, x.shape[1:3])
    dW, db = ref.wgrad_ref(x, g, k, s, p)
    assert y.shape == g.shape and dx.shape == x.shape and dW.shape == W.shape
    a, b, c = _dot(y, g), _dot(x, dx), _dot(W, dW)
    assert _rel(a, b) <= 1e-12 and _rel(a, c) <= 1e-12, (a, b, c)
    assert torch.equal(db, g.double().sum(dim=(0, 1, 2)))


@pytest.mark.parametrize("delta", ref.EXTRA_DELTAS)
@pytest.mark.parametrize("case", ref.EXTRA_CASES)
def test_extra_row_cases_adjoints_and_live_taps(case, delta):
    B, Hi, Wi, cin, cout, k, s, p = case
    out_hw = ref.extra_out_hw(case, delta)
    assert out_hw == (ref.min_out(Hi, k, s, p) + delta[0], ref.min_out(Wi, k, s, p) + delta[1])
    x, W, b, g = ref.rand_case(1, B, Hi, Wi, cin, cout, k, out_hw)
    _adjoint_identities(x, W, g, k, s, p, out_hw)
    # the extra row / column has an in-image tap: it is not the bias alone, and it changes when only the last input row / column does
    y = ref.conv_ref(x, W, b, k, s, p, out_hw)
    if delta[0]:
        assert (out_hw[0] - 1) * s - p <= Hi - 1
        assert float((y[:, -1] - b.double()).abs().max()) > 1e-2
        x2 = x.clone(); x2[:, -1] += 1.0
        assert float((ref.conv_ref(x2, W, b, k, s, p, out_hw)[:, -1] - y[:, -1]).abs().max()) > 1e-2
    if delta[1]:
        assert (out_hw[1] - 1) * s - p <= Wi - 1
        assert float((y[:, :, -1] - b.double()).abs().max()) > 1e-2
        x2 = x.clone(); x2[:, :, -1] += 1.0
        assert float((ref.conv_ref(x2, W, b, k, s, p, out_hw)[:, :, -1] - y[:, :, -1]).abs().max()) > 1e-2


@pytest.mark.parametrize("Hi,Wi,k,s,p", [(13, 17, 3, 2, 1), (12, 14, 4, 2, 1), (9, 11, 3, 1, 1), (13, 15, 7, 2, 3)])
def test_symmetric_pad_size_is_torchs_padded_conv(Hi, Wi, k, s, p):
    """where the symmetric-pad window ends on the padded image's last row, the explicit-size graph is F.conv2d(padding=p)"""
    assert (Hi + 2 * p - k) % s == 0 and (Wi + 2 * p - k) % s == 0
    hw = (ref.min_out(Hi, k, s, p), ref.min_out(Wi, k, s, p))
    x, W, b, _ = ref.rand_case(5, 2, Hi, Wi, 8, 12, k, hw)
    y0 = torch.nn.functional.conv2d(x.double().permute(0, 3, 1, 2), W.double().permute(3, 2, 0, 1), b.double(), stride=s, padding=p)
    y = ref.conv_ref(x, W, b, k, s, p, hw)
    assert y.shape == y0.permute(0, 2, 3, 1).shape
    assert float((y - y0.permute(0, 2, 3, 1)).abs().max()) <= 1e-13 * float(y0.abs().max())


@pytest.mark.parametrize("delta", ref.EXTRA_DELTAS)
@pytest.mark.parametrize("case", [c for c in ref.EXTRA_CASES if c[5:] == (4, 2, 1)])
def test_cropped_conv_transpose_is_the_input_gradient(case, delta):
    """k 4, stride 2, pad 1: the input gradient of the conv is DeConv2dLayer's forward, filter [4,4,cout_of_deconv,cin_of_deconv] =
    the conv's [k,k,cin,cout], cropped to the conv's input size"""
    B, Hi, Wi, cin, cout, k, s, p = case
    out_hw = ref.extra_out_hw(case, delta)
    # "23 <- 12": ceil(Hi / 2) rows in, the transposed conv's 2 * rows cropped by one.  (Without the extra row an odd image keeps a
    # last row that only the last window's last tap reaches: -1.)
    assert (2 * out_hw[0] - Hi) in (-1, 0, 1) and (2 * out_hw[1] - Wi) in (-1, 0, 1)
    _, W, _, g = ref.rand_case(2, B, Hi, Wi, cin, cout, k, out_hw)
    bias = torch.randn(cin, generator=torch.Generator().manual_seed(3))
    a = ref.dgrad_ref(g, W, bias, k, s, p, (Hi, Wi))
    b = ref.deconv_ref(g, W, bias, (Hi, Wi))
    assert a.shape == b.shape == (B, Hi, Wi, cin)
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


@pytest.mark.parametrize("case", ref.PHASE_CASES)
def test_phase_plan_cases_side_of_the_threshold_and_adjoints(case):
    B, Hi, Wi, cin, cout, k, p, ghw, tiles, per_phase = case
    assert ref.dgrad_plan_tiles(B, Hi, Wi, cin, k, p) == tiles
    assert (tiles > ref.PHASE_THRESHOLD) == per_phase
    out_hw = ref.phase_out_hw(case)
    for got, n in zip(out_hw, (Hi, Wi)):
        assert got - ref.min_out(n, k, 2, p) == (1 if ghw else 0)
    x, W, _, g = ref.rand_case(4, B, Hi, Wi, cin, cout, k, out_hw)
    _adjoint_identities(x, W, g, k, 2, p, out_hw)
    if ghw:                                              # the extra row and column read the last image row / column
        y = ref.conv_ref(x, W, None, k, 2, p, out_hw)
        assert float(y[:, -1].abs().max()) > 1e-2 and float(y[:, :, -1].abs().max()) > 1e-2


def test_the_threshold_is_between_180_and_184():
    """256 tiles is the last merged launch: 180x180 has exactly 256, one more tile per parity crosses it"""
    assert ref.dgrad_plan_tiles(1, 180, 180, 8, 3, 1) == ref.PHASE_THRESHOLD
    assert ref.dgrad_plan_tiles(1, 182, 182, 8, 3, 1) > ref.PHASE_THRESHOLD
    # the Trainer's conv2 / conv3 at the reference's training shape and the benchmark's take one launch per phase
    assert ref.dgrad_plan_tiles(10, 192, 256, 64, 5, 2) > ref.PHASE_THRESHOLD and ref.dgrad_plan_tiles(8, 128, 128, 128, 5, 2) > ref.PHASE_THRESHOLD
    # ... and the largest odd-k stride-2 input gradient of the 2x192x256 Trainer tests does not (conv2: 4 x 48 tiles)
    assert ref.dgrad_plan_tiles(2, 96, 128, 64, 5, 2) == 192
