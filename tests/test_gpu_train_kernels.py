"""Three kernels of the training step on their own, through the C entry points, against tests/train_kernels_ref.py:
`vstab_column_sum` and `vstab_pf2_taps_backward` EXACTLY (small integers in float32: every partial sum is below 2^24, addition is
exact in any order, so one dropped or doubled row shows), `vstab_adam_step` within four times the error of its float32 restatement
(train_kernels_ref's docstring).  Inputs the kernels must not read are NaN, outputs they must write are NaN beforehand, and what lies
behind a buffer's stated end is checked afterwards."""
import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime
from tests import train_kernels_ref as ref

pytestmark = pytest.mark.gpu
NAN = float("nan")


def _ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, shape, generator=torch.Generator().manual_seed(seed)).float()


# ----------------------------------------------------------------------------- vstab_column_sum
# reduce_chunks(rows, C) = clamp(rows / 128, 1, max(8, 768 / column blocks)) chunks of ceil(rows / chunks) rows; Cp = the power of two
# >= C up to 64, a wave reads 64 / Cp rows at once; the final stage's wave w adds chunks w, w + 16, ..., four at a time while k + 48 < chunks
COLUMN_SUM_CASES = [
    (1, 4, 0, 2),                # one chunk, one row: 31 of a wave's 32 sub-rows idle
    (127, 4, 0, 2),              # one chunk; Cp = 2, 32 rows per wave, row tail
    (129, 8, 3, 3),              # Cp = 4 with an idle lane in every group; unaligned c_off
    (1000, 24, 4, 20),           # Cp = 32, 7 chunks
    (1031, 64, 0, 64),           # Cp = 64, 8 chunks
    (2049, 72, 4, 65),           # the second column block holds one channel
    (5000, 200, 0, 196),         # four column blocks, the last ragged
    (12801, 640, 0, 640),        # 10 column blocks, 76 chunks: the final stage's four-in-flight loop and its tail
    (98311, 4, 0, 2),            # the workload's 768 chunks of 129 rows: chunk 762 holds 13 rows, chunks 763..767 none
]
GUARD = 4096


def _column_sum(L, g, rows, cs, c_off, C, out, accumulate, scratch, scratch_bytes):
    return L.vstab_column_sum(g.data_ptr(), rows, cs, c_off, C, out.data_ptr() if out is not None else None, accumulate,
                              scratch.data_ptr(), scratch_bytes, runtime.stream_ptr())


def _column_sum_input(values, cs, c_off, C):
    g = torch.full((values.shape[0], cs), NAN)
    g[:, c_off:c_off + C] = values
    return g.cuda()


@pytest.mark.parametrize("rows,cs,c_off,C", COLUMN_SUM_CASES)
def test_column_sum_exact(rows, cs, c_off, C):
    L = _lib.lib()
    g = _column_sum_input(_ints((rows, C), -4, 4, rows + C), cs, c_off, C)
    want = ref.column_sum_ref(g.cpu(), c_off, C)
    assert float(want.abs().max()) < 2 ** 24
    nbytes = int(L.vstab_column_sum_scratch_bytes(rows, C))
    assert nbytes > 0
    scratch = torch.full((nbytes + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((C + 16,), NAN, device="cuda")
    out[C:] = 7.0
    assert _column_sum(L, g, rows, cs, c_off, C, out, 0, scratch, nbytes) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:C].cpu(), want.float())
    prior = _ints((C,), -1000, 1000, C).cuda()
    out[:C] = prior
    assert _column_sum(L, g, rows, cs, c_off, C, out, 1, scratch, nbytes) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:C].cpu(), (want + prior.cpu().double()).float())
    assert bool((out[C:] == 7.0).all())                                     # nothing written past out[C]
    assert bool((scratch[nbytes:] == 0xA5).all())                           # nor past the scratch size the library asked for
    # the summation order is fixed: random data twice gives the same bits (and the right sum, to a sum's accuracy)
    gr = _column_sum_input(torch.randn(rows, C, generator=torch.Generator().manual_seed(rows)), cs, c_off, C)
    a, b = torch.full((C,), NAN, device="cuda"), torch.full((C,), NAN, device="cuda")
    assert _column_sum(L, gr, rows, cs, c_off, C, a, 0, scratch, nbytes) == 0
    scratch.fill_(0x5A)
    assert _column_sum(L, gr, rows, cs, c_off, C, b, 0, scratch, nbytes) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    # rows - 1 additions of at most 2^-24 relative error each, whatever their order
    slack = rows * ref.EPS32 * gr.cpu()[:, c_off:c_off + C].double().abs().sum(dim=0)
    assert bool(((a.cpu().double() - ref.column_sum_ref(gr.cpu(), c_off, C)).abs() <= slack).all())


def test_column_sum_rejects_bad_arguments():
    L = _lib.lib()
    rows, cs, c_off, C = 129, 8, 3, 3
    g = _column_sum_input(_ints((rows, C), -4, 4, 1), cs, c_off, C)
    nbytes = int(L.vstab_column_sum_scratch_bytes(rows, C))
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    out = torch.full((C,), 7.0, device="cuda")
    assert L.vstab_column_sum_scratch_bytes(0, C) == 0 and L.vstab_column_sum_scratch_bytes(rows, 0) == 0
    assert _column_sum(L, g, rows, cs, c_off, C, out, 0, scratch, nbytes - 1) < 0           # scratch one byte short
    assert b"scratch" in L.vstab_last_error(None)
    assert _column_sum(L, g, rows, cs, 6, C, out, 0, scratch, nbytes) < 0                   # c_off + C > cs
    assert _column_sum(L, g, 0, cs, c_off, C, out, 0, scratch, nbytes) < 0                  # no rows
    assert _column_sum(L, g, rows, cs, c_off, C, None, 0, scratch, nbytes) < 0              # NULL out
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert _column_sum(L, g, rows, cs, c_off, C, out, 0, scratch, nbytes) == 0              # and the same call in order is taken
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref.column_sum_ref(g.cpu(), c_off, C).float())


# ----------------------------------------------------------------------------- vstab_pf2_taps_backward
def _taps_backward(L, g, cs_g, B, H, W, dT, h2, w2):
    return L.vstab_pf2_taps_backward(g.data_ptr(), cs_g, B, H, W, dT.data_ptr(), h2, w2, runtime.stream_ptr())


@pytest.mark.parametrize("B,h2,w2,H,W,cs_g", ref.PF2_CASES)
def test_pf2_taps_backward_exact_and_adjoint_of_the_forward_kernel(B, h2, w2, H, W, cs_g):
    """The backward finds the output rows of a source row inside rc +- span, both derived from 1 / sy in float32: the shapes cover the
    identity map, the network's 4x, a 10x and a shrinking ratio and two downsampling heads (where the forward takes its direct-gather
    kernel).  A window one row short anywhere loses gradient, and the exact comparison sees it."""
    L = _lib.lib()
    oh, ow = H - 2, W - 2
    gv = _ints((B, oh, ow, 2), -3, 3, h2 * 100 + W)
    g = torch.full((B, oh, ow, cs_g), NAN)
    g[..., :2] = gv
    g = g.cuda()
    n = B * h2 * w2 * 32
    buf = torch.full((n + 64,), NAN, device="cuda")
    buf[n:] = 7.0
    dT = buf[:n].view(B, h2, w2, 32)
    assert _taps_backward(L, g, cs_g, B, H, W, dT, h2, w2) == 0
    torch.cuda.synchronize()
    got = dT.cpu()
    assert bool(torch.isfinite(got).all())
    assert bool((got[..., 18:] == 0.0).all())
    assert bool((buf[n:] == 7.0).all())
    want = ref.pf2_taps_backward_ref(gv, h2, w2, H, W)
    assert float(want.abs().max()) < 2 ** 24
    assert torch.equal(got, want.float())
    # on the GPU alone: <forward kernel(T), g> == <T, backward kernel(g)>, integers, summed in fp64 on the host.  The forward reads
    # 18 columns of a table row: the others are NaN here
    T = torch.full((B, h2, w2, 32), NAN)
    T[..., :18] = _ints((B, h2, w2, 18), -3, 3, H * 100 + w2)
    h3, w3 = (h2 + 1) // 2, (w2 + 1) // 2
    Td, zero_bias, zero_pf3 = T.cuda(), torch.zeros(2, device="cuda"), torch.zeros(B, h3, w3, 2, device="cuda")
    pf2 = torch.full((B, oh, ow, 2), NAN, device="cuda")
    assert L.vstab_pf2_from_taps(Td.data_ptr(), B, h2, w2, zero_bias.data_ptr(), zero_pf3.data_ptr(), h3, w3, pf2.data_ptr(), H, W,
                                 runtime.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(pf2.cpu(), ref.pf2_tap_gather(T[..., :18].double(), H, W).float())
    lhs = float((pf2.cpu().double() * gv.double()).sum())
    rhs = float((T[..., :18].double() * got[..., :18].double()).sum())
    assert lhs == rhs


def test_pf2_taps_backward_rejects_bad_arguments():
    L = _lib.lib()
    B, h2, w2, H, W = 1, 3, 4, 8, 9
    g = torch.zeros(B, H - 2, W - 2, 2, device="cuda")
    dT = torch.full((B, h2, w2, 32), 7.0, device="cuda")
    assert _taps_backward(L, g, 2, B, 2, W, dT, h2, w2) < 0                 # H = 2: no output row
    assert _taps_backward(L, g, 1, B, H, W, dT, h2, w2) < 0                 # one channel: no (u, v) pair
    assert L.vstab_pf2_taps_backward(None, 2, B, H, W, dT.data_ptr(), h2, w2, runtime.stream_ptr()) < 0
    torch.cuda.synchronize()
    assert bool((dT == 7.0).all())


# ----------------------------------------------------------------------------- vstab_adam_step
@pytest.mark.parametrize("n,b1", ref.ADAM_CASES)
def test_adam_step_four_steps_from_a_running_state(n, b1):
    """One block, the 256 boundary on both sides, a ragged last block of many.  m and v start non-zero, so both decays, both (1 - b)
    factors and the place of eps all act on the result (tests/test_train_kernels_ref_cpu.py shows the bound rejects each of those
    mistakes on these inputs).  Every step is compared with one fp64 step from the state the GPU itself held before it."""
    L = _lib.lib()
    w0, m0, v0, g = ref.adam_case(n, b1)
    pad = 64

    def padded(a, fill):
        return torch.cat([torch.from_numpy(a), torch.full((pad,), fill)]).cuda()

    w, m, v, gd = padded(w0, 3.0), padded(m0, 5.0), padded(v0, 7.0), padded(g[0], 11.0)
    worst = np.zeros(3)
    for t in range(1, ref.ADAM_STEPS + 1):
        gd[:n] = torch.from_numpy(g[t - 1])
        before = tuple(a[:n].cpu().numpy() for a in (w, m, v))
        step = ref.lr_t(ref.ADAM_LR, b1, ref.ADAM_B2, t)
        assert L.vstab_adam_step(w.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), n, step, b1, ref.ADAM_B2, ref.ADAM_EPS,
                                 runtime.stream_ptr()) == 0
        torch.cuda.synchronize()
        after = tuple(a[:n].cpu().numpy() for a in (w, m, v))
        err = ref.adam_errors(after, before, g[t - 1], step, b1, ref.ADAM_B2, ref.ADAM_EPS)
        print(f"adam n={n} b1={b1} t={t}: error in units (w, m, v) = {err}, bound {ref.ADAM_BOUND}")
        worst = np.maximum(worst, err)
        assert all(e <= b for e, b in zip(err, ref.ADAM_BOUND)), (t, err, ref.ADAM_BOUND)
        if n > 3:
            assert after[0][3] != before[0][3]                           # g = 0 but m != 0: the weight still moves
        if n > 17:
            assert after[0][17] == before[0][17] and after[1][17] == 0 and after[2][17] == 0      # all zero: 0 / eps, no NaN
        if n > 200:
            # g^2 is negligible, v stays negligible next to eps^2: the step is lr_t m / eps
            want = float(np.float32(step)) * float(after[1][200]) / float(np.float32(ref.ADAM_EPS))
            assert abs((float(before[0][200]) - float(after[0][200])) / want - 1.0) <= 1e-5
    print(f"adam n={n} b1={b1}: largest error over the four steps {tuple(worst)}")
    for a, fill in ((w, 3.0), (m, 5.0), (v, 7.0), (gd, 11.0)):
        assert bool((a[n:] == fill).all())                                # the tail of the last block writes nothing


def test_adam_step_rejects_bad_arguments():
    L = _lib.lib()
    w, g, m, v = (torch.full((8,), 7.0, device="cuda") for _ in range(4))
    st = runtime.stream_ptr()
    assert L.vstab_adam_step(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0, 1e-3, 0.9, 0.999, 1e-8, st) < 0
    assert L.vstab_adam_step(w.data_ptr(), g.data_ptr(), m.data_ptr(), None, 8, 1e-3, 0.9, 0.999, 1e-8, st) < 0
    torch.cuda.synchronize()
    assert all(bool((a == 7.0).all()) for a in (w, g, m, v))
