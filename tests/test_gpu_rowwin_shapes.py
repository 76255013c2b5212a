"""Every path of the fp32 row-window kernel (csrc/conv_rowwin.hip) at about the smallest geometry that reaches it, through
vstab_conv_rowwin_forward.  The 27-channel 7x7 first layer of the other tests always takes the assembly K loop (six K-tiles per filter
row); these cases run the C++ loop with an odd and an even number of K-tiles per filter row, KH != 7, N < 64, both epilogues, a
channel slice of a wider pixel, and the 128 k + (1..64) column split.

Reference: torch's fp64 conv2d on the CPU plus the activation; tolerance 2e-5 * max|ref| + 1e-6 as in tests/test_gpu_training.py.

    case  B  HxW      Cin cs_w cout k s p cs_y cy_off act | Wo  MB pix_step SEGP K-tiles/row WLEN
    a     2  20x24    4   8    20   3 2 1 24   4      1   | 12  1  8        32   1           536    scalar epilogue (2 WLEN < 64*64)
    b     1  17x70    16  16   62   3 2 1 64   0      2   | 35  1  32       64   2           2080   staged epilogue, partial channel group
    c     4  256x260  16  16   64   3 2 1 64   0      0   | 130 2  32       64   2           4128   one 128-pixel tile + the 64-pixel tail launch
"""
import pytest
import torch
import torch.nn.functional as F

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -777.0        # finite: a stray NaN (the filter's poisoned padding channels) shows as well as a stray number

#        B  H    W    Cin cs_w cout k  s  p  cs_y cy_off act
CASES = {"a_odd_ktiles_scalar_epilogue_slice": (2, 20, 24, 4, 8, 20, 3, 2, 1, 24, 4, 1),
         "b_paired_ktiles_staged_epilogue_ragged": (1, 17, 70, 16, 16, 62, 3, 2, 1, 64, 0, 2),
         "c_two_blocks_per_wave_and_tail_launch": (4, 256, 260, 16, 16, 64, 3, 2, 1, 64, 0, 0)}


def run(x, Wf, b, geom, y):
    B, H, W, Cin, cs_w, cout, k, s, p, cs_y, cy_off, act = geom
    L = _lib.lib()
    n = L.vstab_conv_rowwin_forward_workspace_bytes(B, H, W, Cin, cs_w, cout, k, s, p, cs_y, cy_off, act)
    ws = torch.empty(int(n) + 1024, dtype=torch.uint8, device="cuda")
    code = L.vstab_conv_rowwin_forward(x.data_ptr(), B, H, W, Cin, Wf.data_ptr(), cs_w, cout, b.data_ptr(), k, s, p, y.data_ptr(), cs_y, cy_off,
                                       act, ws.data_ptr(), ws.numel(), None)
    torch.cuda.synchronize()
    return int(n), code


@pytest.mark.parametrize("name", list(CASES))
def test_row_window_kernel_path(name):
    geom = CASES[name]
    B, H, W, Cin, cs_w, cout, k, s, p, cs_y, cy_off, act = geom
    g = torch.Generator().manual_seed(1000 + list(CASES).index(name))
    x = torch.rand(B, H, W, Cin, generator=g)
    Wf = torch.randn(k, k, cs_w, cout, generator=g) / (k * k * Cin) ** 0.5
    Wf[:, :, Cin:, :] = float("nan")                     # the filter's padding channels are never read
    b = torch.randn(cout, generator=g) * 0.1
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    y = torch.full((B, Ho, Wo, cs_y), SENTINEL, dtype=torch.float32, device="cuda")
    n, code = run(x.cuda(), Wf.cuda(), b.cuda(), geom, y)
    assert n > 0                                         # the row-window kernel takes the geometry
    _lib.check(code)
    y = y.cpu()
    inside = y[..., cy_off:cy_off + cout]
    assert bool(torch.isfinite(inside).all())
    assert bool((y[..., :cy_off] == SENTINEL).all()) and bool((y[..., cy_off + cout:] == SENTINEL).all())     # no stray write of any value
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), Wf[:, :, :Cin].double().permute(3, 2, 0, 1), b.double(), stride=s, padding=p).permute(0, 2, 3, 1)
    if act == 1:
        ref = torch.maximum(ref, 0.1 * ref)
    elif act == 2:
        ref = torch.relu(ref)
    err, bound = float((inside.double() - ref).abs().max()), 2e-5 * float(ref.abs().max()) + 1e-6
    print(f"rowwin {name}: max abs err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_row_not_a_multiple_of_four_floats_is_refused_without_a_launch():
    """(W * Cin) % 4 != 0 (25 * 3 floats per row): the query says 0 and the call fails before it launches anything"""
    geom = (1, 20, 25, 3, 4, 16, 3, 2, 1, 16, 0, 1)
    g = torch.Generator().manual_seed(1003)
    x = torch.rand(1, 20, 25, 3, generator=g).cuda()
    Wf = (torch.randn(3, 3, 4, 16, generator=g) / 27 ** 0.5).cuda()
    b = (torch.randn(16, generator=g) * 0.1).cuda()
    y = torch.full((1, 10, 13, 16), SENTINEL, dtype=torch.float32, device="cuda")
    n, code = run(x, Wf, b, geom, y)
    assert n == 0 and code < 0
    assert b"does not take this geometry" in _lib.lib().vstab_last_error(None)
    assert bool((y == SENTINEL).all())
