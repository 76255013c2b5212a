"""The 16 Winograd-domain GEMMs of a 3x3 stride-1 stage as streams of positions (csrc/wino_gemm_stream.hip; the K loop, the seams between
positions and the stores of a finished tile are the generated block VSTAB_GEMM_STREAM_ASM, tools/gen_conv_kloop.py's GemmStreamGen), run by
themselves through vstab_wino_domain_gemm: M[b][xi] = V[b][xi] . U[xi] on the full tensor against an fp64 matmul, on exact integers, bit for
bit against the tiled launch it replaces (wino_gemm_stream.hip's "bit-identical to it"), with guard bands around M, and inside the network
under VSTAB_PLAN_NO_WINO_STREAM.  The kernel's grid is always 512 workgroups, so the cases are the smallest shapes it takes: every number
of positions per workgroup, 4 / 6 / 8 / 16 / 32 K-tiles per position, one column tile, one sample, one row tile per sample.  The transforms
around the GEMM are tests/test_gpu_train_conv_edges.py's (vstab_conv3x3_winograd); the operand layout both forms read is pinned to the
inference path's packing by tests/test_host_plan.py (blocked_pack_np) and, for the device-side packing, below."""
import ctypes as C

import numpy as np
import pytest
import torch

import coupe.optical_flow_based_deep_video_stabilization_amd as vs
from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, runtime, weights as wts
from tests.test_host_plan import STREAM_CASES, blocked_pack_np

pytestmark = pytest.mark.gpu
NO_WINO_STREAM = 64
GUARD = 4096                    # floats on either side of M
GUARD_BITS = 0x4B1D5EED         # what they hold (as int32)
TILED, STREAM = 0, 1
KEYS = ("predict_flow6", "predict_flow5", "predict_flow4", "predict_flow3", "predict_flow2")


def _workspace(B, T, cin, cout):
    n = _lib.lib().vstab_wino_domain_gemm_workspace_bytes(B, T, cin, cout)
    assert n > 0, (B, T, cin, cout)
    return torch.empty(int(n), dtype=torch.uint8, device="cuda")


def _guarded(n):
    """an int32 buffer of GUARD + n + GUARD words: the guards hold GUARD_BITS, the n floats between them NaN; returns (buffer, M view)"""
    buf = torch.full((n + 2 * GUARD,), GUARD_BITS, dtype=torch.int32, device="cuda")
    M = buf[GUARD:GUARD + n].view(torch.float32)
    M.fill_(float("nan"))
    return buf, M


def _gemm(V, U, shape, form, ws=None):
    """one call on a NaN-filled, guarded M; returns (M [B,16,T,cout], the guarded buffer, the workspace)"""
    B, T, cin, cout = shape
    ws = _workspace(B, T, cin, cout) if ws is None else ws
    buf, M = _guarded(B * 16 * T * cout)
    _lib.check(_lib.lib().vstab_wino_domain_gemm(V.data_ptr(), U.data_ptr(), M.data_ptr(), B, T, cin, cout, form, ws.data_ptr(), ws.numel(), None))
    torch.cuda.synchronize()
    return M.view(B, 16, T, cout), buf, ws


def _guards_intact(buf):
    return bool((buf[:GUARD] == GUARD_BITS).all()) and bool((buf[-GUARD:] == GUARD_BITS).all())


class _Case:
    """the random problem of one shape, drawn once, and what the two forms make of it (nothing here is modified by a test)"""

    def __init__(self, B, T, cin, cout, P):
        self.shape, self.P = (B, T, cin, cout), P
        g = torch.Generator().manual_seed(B * 100003 + T * 101 + cin * 7 + cout)
        self.V = torch.randn(B, 16, T, cin, generator=g)
        self.U = torch.randn(16, cin, cout, generator=g) / cin ** 0.5
        self.Vd, self.Ud = self.V.cuda(), self.U.cuda()
        self.stream, self.stream_buf, self.ws = _gemm(self.Vd, self.Ud, self.shape, STREAM)
        self.tiled, self.tiled_buf, _ = _gemm(self.Vd, self.Ud, self.shape, TILED)


@pytest.fixture(scope="module", params=STREAM_CASES, ids=lambda c: "B%d-T%d-%dto%d-P%d" % c)
def case(request):
    B, T, cin, cout, P = request.param
    assert _lib.lib().vstab_host_wino_stream_positions(B, T, cin, cout) == P
    c = _Case(B, T, cin, cout, P)
    yield c
    del c
    torch.cuda.empty_cache()


def test_stream_form_vs_fp64_matmul(case):
    """ref[b, xi] = V[b, xi] . U[xi] in fp64 on the CPU, every element of M; the tolerance is tests/test_gpu_kloop.py's for this MFMA
    kernel family.  (profiles/README.md lists the measured maxima per case.)"""
    B, T, cin, cout = case.shape
    Ud = case.U.double()
    ref_max, err_s, err_t = [], [], []
    for b in range(B):                                                       # a sample at a time: the fp64 tensors stay small
        ref = torch.bmm(case.V[b].double(), Ud)                              # [16, T, cout]
        ref_max.append(ref.abs().max())
        err_s.append((case.stream[b].double().cpu() - ref).abs().max())
        err_t.append((case.tiled[b].double().cpu() - ref).abs().max())
    # (torch's max hands a NaN on, Python's would drop it: an unwritten element of M fails the comparison below)
    ref_max, err_s, err_t = (float(torch.stack(v).max()) for v in (ref_max, err_s, err_t))
    tol = 2e-5 * ref_max + 1e-6
    print(f"wino_domain_gemm B={B} T={T} {cin}->{cout} P={case.P}: max|ref| {ref_max:.4f} max err stream {err_s:.3e} tiled {err_t:.3e} tol {tol:.3e}")
    assert err_s <= tol, (err_s, tol)
    assert err_t <= tol, (err_t, tol)


def test_exact_integers(case):
    """V in [-3, 3], U in [-2, 2]: every product and every partial sum is an integer below 6 * cin <= 6144 < 2^24, exact in fp32 in any
    order -- so the reference (an fp32 matmul on the CPU) is exact, and a dropped, doubled or misplaced K-tile or position cannot hide in
    a tolerance"""
    B, T, cin, cout = case.shape
    g = torch.Generator().manual_seed(cin * 13 + T + B)
    V = torch.randint(-3, 4, (B, 16, T, cin), generator=g).float()
    U = torch.randint(-2, 3, (16, cin, cout), generator=g).float()
    ref = torch.matmul(V, U)                                                 # [B, 16, T, cout]
    assert float(ref.abs().max()) <= 6 * cin and bool((ref == ref.round()).all())
    Vd, Ud = V.cuda(), U.cuda()
    for form in (STREAM, TILED):
        M, buf, _ = _gemm(Vd, Ud, case.shape, form)                          # (a workspace of its own: case.ws keeps the random operand)
        assert torch.equal(M.cpu(), ref), form
        assert _guards_intact(buf), form


def test_stream_form_is_bit_identical_to_the_tiled_launch(case):
    """same K-tile order, same MFMA order per accumulator, same `+ 0.0` of the zero bias: the claim of wino_gemm_stream.hip's header"""
    assert torch.equal(case.stream, case.tiled)


def test_writes_all_of_m_and_nothing_else(case):
    """M was NaN before the call and sits between two guard bands: every element is written, none outside, and a second run on the
    same operands gives the same bits"""
    for form, M, buf in ((STREAM, case.stream, case.stream_buf), (TILED, case.tiled, case.tiled_buf)):
        assert not bool(torch.isnan(M).any()), form
        assert _guards_intact(buf), form
        again, buf2, _ = _gemm(case.Vd, case.Ud, case.shape, form, case.ws)
        assert torch.equal(again, M) and _guards_intact(buf2), form


def test_device_packed_operand_is_the_blocked_layout(case):
    """both forms read U from the head of the workspace, packed on the device; it is the layout vstab_load_weights packs a stage's
    operand in (tests/test_host_plan.py: blocked_pack_np against pack_winograd), position by position"""
    B, T, cin, cout = case.shape
    wpk = case.ws[:16 * cin * cout * 4].view(torch.float32).cpu().numpy().reshape(16, cin // 32, cout, 32)
    U = case.U.numpy()
    for xi in range(16):
        assert np.array_equal(wpk[xi], blocked_pack_np(U[xi])), xi


def test_refusals():
    L = _lib.lib()
    B, T, cin, cout = 4, 256, 512, 512                                       # the stream form takes it with 2 positions per workgroup
    V = torch.zeros(B, 16, T, cin, device="cuda")
    U = torch.zeros(16, cin, cout, device="cuda")
    ws = _workspace(B, T, cin, cout)
    buf, M = _guarded(B * 16 * T * cout)

    def call(v=V.data_ptr(), u=U.data_ptr(), m=M.data_ptr(), shape=(B, T, cin, cout), form=STREAM, w=ws.data_ptr(), wn=ws.numel()):
        return L.vstab_wino_domain_gemm(v, u, m, *shape, form, w, wn, None)

    # a shape the stream form does not take: refused for form 1, and the launcher's rule is the one that says so
    for shape in ((1, 128, 128, 64), (4, 192, 512, 512), (4, 256, 64, 512), (4, 256, 160, 512), (3, 256, 512, 512)):
        assert L.vstab_host_wino_stream_positions(*shape) == 0
        assert call(shape=shape) == -1, shape                                # VSTAB_E_SHAPE
    assert call(shape=(B, T, cin, 96)) == -1 and call(shape=(B, T, 48, cout)) == -1 and call(form=2) == -1 and call(shape=(0, T, cin, cout)) == -1
    assert call(shape=(64, 4096, 128, 64), form=TILED) == -1                 # V would be 2 GiB
    assert L.vstab_wino_domain_gemm_workspace_bytes(64, 4096, 128, 64) == 0 and L.vstab_wino_domain_gemm_workspace_bytes(B, T, cin, 96) == 0
    # the launcher reached with a number of positions that is not the rule's
    assert L.vstab_host_wino_stream_positions(B, T, cin, cout) == 2
    for P in (0, 1, 3, 4, 8, 16, 32):
        assert L.vstab_wino_gemm_stream_launch(V.data_ptr(), ws.data_ptr(), M.data_ptr(), B, T, cin, cout, P, None) == -1, P
    assert L.vstab_wino_gemm_stream_launch(V.data_ptr(), ws.data_ptr(), M.data_ptr(), 3, T, cin, cout, 2, None) == -1
    assert L.vstab_wino_gemm_stream_launch(None, ws.data_ptr(), M.data_ptr(), B, T, cin, cout, 2, None) == -6
    assert L.vstab_wino_gemm_stream_launch(V.data_ptr(), ws.data_ptr() + 4, M.data_ptr(), B, T, cin, cout, 2, None) == -2
    # NULL, misaligned, short workspace
    for form in (STREAM, TILED):
        assert call(v=None, form=form) == -6 and call(u=None, form=form) == -6 and call(m=None, form=form) == -6 and call(w=None, form=form) == -6
        assert call(v=V.data_ptr() + 4, form=form) == -2 and call(u=U.data_ptr() + 8, form=form) == -2 and call(m=M.data_ptr() + 4, form=form) == -2
        assert call(w=ws.data_ptr() + 16, form=form) == -2                   # 16-byte but not 256-byte aligned
        assert call(wn=ws.numel() - 1, form=form) == -4                      # VSTAB_E_NOMEM
    torch.cuda.synchronize()
    assert bool(torch.isnan(M).all()) and _guards_intact(buf)                # none of the refused calls launched anything that wrote
    # and the same arguments, unbroken, run
    assert call() == 0 and call(form=TILED) == 0
    torch.cuda.synchronize()
    assert float(M.abs().max()) == 0.0 and _guards_intact(buf)


def test_network_with_and_without_the_stream_form_is_bit_identical():
    """one forward at B = 4 of 512x512x27 with the default plan -- conv3_1 (4 positions per workgroup) and conv4_1 (2) run on the stream
    kernel -- and one under VSTAB_PLAN_NO_WINO_STREAM, where both take the tiled launch (128x128 tiles for conv3_1, 128x64 for conv4_1:
    a tile shape changes no sum).  The Winograd-domain descriptor is always built without split-K (conv_desc_planes: ksplit = 1; what
    vstab_host_layer_plan reports for these stages is the direct form's descriptor, which is not launched), so nothing here reassociates a
    sum: conv3, conv4 and all five flows are equal bit for bit, with no plan-to-plan bound."""
    B, H, W = 4, 512, 512
    L = _lib.lib()
    out = (C.c_int32 * 200)()
    for layer in (3, 5):                                                     # conv3_1, conv4_1
        plans = []
        for flags in (0, NO_WINO_STREAM):
            n = L.vstab_host_layer_plan_pinned(0, flags, B, H, W, 27, layer, out, 200)
            assert n > 0 and out[25] == 1                                    # runs in Winograd form
            plans.append(list(out[:n]))
        assert plans[0] == plans[1]                                          # the plan does not know about the stream form
    assert L.vstab_host_wino_stream_positions(B, 1024, 256, 256) == 4 and L.vstab_host_wino_stream_positions(B, 256, 512, 512) == 2
    runtime.reset()
    try:
        vs.assign_weights(wts.synthetic_weights(seed=3, cin=27, random_bn=True, flow_gain=2.0))
        ctx = runtime.get_context()
        g = torch.Generator(device="cuda").manual_seed(41)
        feats = torch.rand(B, H, W, 27, generator=g, device="cuda")
        runs = []
        for flags in (0, NO_WINO_STREAM):
            ctx.set_plan_flags(flags)
            ctx.profile(True)
            flows = vs.flownetS_pyramid(feats, B)
            torch.cuda.synchronize()
            names = ctx.profile_kernel_names()
            ctx.profile(False)
            ints = ctx.internals(B, H, W, 27)
            runs.append((names, {k: flows[k].clone() for k in KEYS}, {k: ints[k].clone() for k in ("conv3", "conv4")}))
        (na, fa, ia), (nb, fb, ib) = runs
        slots = {s: i for i, s in enumerate(ctx.LAUNCH_SLOTS)}
        for s in ("conv3_1", "conv4_1"):
            assert na[slots[s]] == "wino_gemm_stream_kernel", (s, na[slots[s]])
            assert "wino_gemm_stream" not in nb[slots[s]] and "conv_mfma_kernel" in nb[slots[s]], (s, nb[slots[s]])
        assert "wino_gemm_stream_kernel" not in nb
        assert [n for i, n in enumerate(na) if i not in (slots["conv3_1"], slots["conv4_1"])] == \
               [n for i, n in enumerate(nb) if i not in (slots["conv3_1"], slots["conv4_1"])]
        for k in ("conv3", "conv4"):
            assert float(ia[k].abs().max()) > 0 and torch.equal(ia[k], ib[k]), k
        for k in KEYS:
            assert torch.equal(fa[k], fb[k]), k
    finally:
        runtime.reset()
