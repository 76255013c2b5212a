"""Plain float64 references of the training step's three convolution entry points (`vstab_conv_forward`, `vstab_conv_dgrad`,
`vstab_conv_wgrad`) with an EXPLICIT output size, and the case tables that tests/test_train_conv_ref_cpu.py (no GPU) and
tests/test_gpu_train_conv_edges.py share.  NHWC tensors, HWIO filters, torch on the CPU.

The library takes one more output row / column than floor((Hi + 2 pad - k) / stride) + 1 (TF SAME on an odd size; the transposed
conv cropped to its skip's size).  Here that is zero padding `pad` at the top / left and whatever the last window needs at the
bottom / right, followed by a VALID conv; the two gradients are torch autograd through that very graph."""
import torch
import torch.nn.functional as F


def min_out(n: int, k: int, s: int, p: int) -> int:
    """the symmetric-pad output size of an axis"""
    return (n + 2 * p - k) // s + 1


def _graph(x_nchw, w_oihw, k, s, p, out_hw):
    Ho, Wo = out_hw
    Hi, Wi = x_nchw.shape[2], x_nchw.shape[3]
    pb, pr = (Ho - 1) * s + k - Hi - p, (Wo - 1) * s + k - Wi - p
    assert pb >= 0 and pr >= 0, "the last window must reach the end of the image"
    return F.conv2d(F.pad(x_nchw, (p, pr, p, pb)), w_oihw, stride=s, padding=0)


def conv_ref(x, W, bias, k, s, p, out_hw):
    """y [B,Ho,Wo,cout] = conv(x [B,Hi,Wi,cin], W [k,k,cin,cout]) + bias (None: no bias), float64"""
    y = _graph(x.double().permute(0, 3, 1, 2), W.double().permute(3, 2, 0, 1), k, s, p, out_hw).permute(0, 2, 3, 1)
    assert tuple(y.shape[1:3]) == tuple(out_hw)
    return (y if bias is None else y + bias.double()).contiguous()


def dgrad_ref(g, W, bias, k, s, p, in_hw):
    """d <conv_ref(x), g> / dx [B,Hi,Wi,cin] (+ bias [cin], the transposed-conv layer's own) for g [B,Ho,Wo,cout]; the output size
    of the conv is g's"""
    B, Ho, Wo, _ = g.shape
    x = torch.zeros(B, W.shape[2], in_hw[0], in_hw[1], dtype=torch.float64, requires_grad=True)
    _graph(x, W.double().permute(3, 2, 0, 1), k, s, p, (Ho, Wo)).backward(g.double().permute(0, 3, 1, 2))
    dx = x.grad.permute(0, 2, 3, 1)
    return (dx if bias is None else dx + bias.double()).contiguous()


def wgrad_ref(x, g, k, s, p):
    """(d <conv_ref(x), g> / dW [k,k,cin,cout], the bias gradient g.sum((0,1,2)))"""
    B, Ho, Wo, cout = g.shape
    W = torch.zeros(cout, x.shape[3], k, k, dtype=torch.float64, requires_grad=True)
    _graph(x.double().permute(0, 3, 1, 2), W, k, s, p, (Ho, Wo)).backward(g.double().permute(0, 3, 1, 2))
    return W.grad.permute(2, 3, 1, 0).contiguous(), g.double().sum(dim=(0, 1, 2))


def deconv_ref(x, Wd, bias, out_hw):
    """DeConv2dLayer (4x4, stride 2, SAME) of x [B,h,w,cin] with the filter Wd [4,4,cout,cin], cropped to out_hw: torch's own
    transposed conv, independent of the graph above.  (output_padding = 1 keeps row 2h / column 2w, which the last window's last
    tap still reaches: an out_hw of 2h + 1 is the symmetric-pad size of an odd image.)"""
    y = F.conv_transpose2d(x.double().permute(0, 3, 1, 2), Wd.double().permute(3, 2, 0, 1), stride=2, padding=1, output_padding=1)
    assert 0 <= y.shape[2] - out_hw[0] <= 2 and 0 <= y.shape[3] - out_hw[1] <= 2
    y = y[:, :, :out_hw[0], :out_hw[1]].permute(0, 2, 3, 1)
    assert tuple(y.shape[1:3]) == tuple(out_hw)
    return (y if bias is None else y + bias.double()).contiguous()


def act_ref(y, act, y0=None):
    """the epilogues of vstab_conv_forward: 0 none, 1 leaky relu 0.1, 2 relu, 3 add to what was in y"""
    if act == 1:
        return torch.maximum(y, 0.1 * y)
    if act == 2:
        return torch.relu(y)
    if act == 3:
        return y + y0.double()
    return y


def rand_case(seed, B, Hi, Wi, cin, cout, k, out_hw):
    """float32 (x, W, bias, g): unit normal tensors, the filter scaled by 1 / sqrt(k k cin)"""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Hi, Wi, cin, generator=gen)
    W = torch.randn(k, k, cin, cout, generator=gen) / (k * k * cin) ** 0.5
    b = torch.randn(cout, generator=gen)
    g = torch.randn(B, out_hw[0], out_hw[1], cout, generator=gen)
    return x, W, b, g


# ----------------------------------------------------------------------------- A. one more output row / column
# (B, Hi, Wi, cin, cout, k, s, p).  Every extra row / column has an in-image tap (k=3, s=2, p=1 on an ODD size would read padding only).
EXTRA_CASES = [
    (2, 13, 17, 16, 24, 4, 2, 1),        # adjoint of the deconv, odd size
    (2, 12, 14, 16, 24, 3, 2, 1),        # odd k on an even size: the extra row reads row 11
    (1, 12, 16, 64, 128, 5, 2, 2),       # conv3-like, 128-column tile
    (1, 12, 14, 8, 8, 7, 2, 3),          # 7x7
    (2, 11, 13, 8, 16, 4, 2, 1),         # the deconv itself: input gradient = DeConv2dLayer 16 -> 8 of a 6x7 map cropped to 11x13
]
EXTRA_DELTAS = [(1, 1), (1, 0), (0, 1)]


def extra_out_hw(case, delta):
    _, Hi, Wi, _, _, k, s, p = case
    return min_out(Hi, k, s, p) + delta[0], min_out(Wi, k, s, p) + delta[1]


# ----------------------------------------------------------------------------- B. odd-k stride-2 input gradients: merged / per-phase plan
# (B, Hi, Wi, cin, cout, k, p, gout_hw or None = the symmetric-pad size, tiles of dgrad_plan, one launch per phase?)
PHASE_THRESHOLD = 256
PHASE_CASES = [
    (1, 180, 180, 8, 8, 3, 1, None, 256, False),          # the last size of the merged launch
    (1, 184, 184, 8, 8, 3, 1, None, 268, True),
    (1, 185, 183, 8, 8, 3, 1, None, 267, True),           # four different grids
    (1, 185, 183, 8, 8, 5, 2, None, 267, True),           # 3 / 2 taps per axis
    (1, 184, 184, 8, 8, 3, 1, (93, 93), 268, True),       # and the extra row / column
    (2, 64, 64, 256, 8, 3, 1, None, 128, False),          # merged, two column blocks
    (2, 96, 96, 256, 8, 3, 1, None, 288, True),           # per phase, two column blocks
    (1, 185, 183, 8, 132, 3, 1, None, 267, True),         # reductions of 2..4 K-tiles, another one for each phase
]


def phase_out_hw(case):
    _, Hi, Wi, _, _, k, p, ghw, _, _ = case
    return tuple(ghw) if ghw else (min_out(Hi, k, 2, p), min_out(Wi, k, 2, p))


def dgrad_plan_tiles(B, Hi, Wi, cin, k, p):
    """The 128-row tiles that plan_dgrad (csrc/train_conv_api.cpp) counts for an odd-k stride-2 input gradient: the output pixels of
    parity (py, px) form one GEMM of B*Hg*Wg rows and cin columns (padded to the column tile: 128 from 128 columns up, 64 above 32,
    else 32).  More than PHASE_THRESHOLD of them run as one launch per parity."""
    assert k & 1
    BN = 128 if cin >= 128 else (64 if cin > 32 else 32)
    npad = (cin + BN - 1) // BN * BN
    tiles = 0
    for py in range(2):
        for px in range(2):
            nty, ntx = (k - ((py + p) & 1) + 1) // 2, (k - ((px + p) & 1) + 1) // 2
            Hg, Wg = (Hi - py + 1) // 2, (Wi - px + 1) // 2
            if min(Hg, Wg, nty, ntx) < 1:
                continue
            tiles += (B * Hg * Wg + 127) // 128 * (npad // BN)
    return tiles
