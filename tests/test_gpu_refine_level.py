"""A refinement level's two hand-written pieces by themselves, each against a plain float64 reference (tests/refine_level_ref.py, pinned on
the CPU by tests/test_refine_level_ref_cpu.py):

  * the 4x4 stride-2 transposed convolution in Winograd F(2x2,2x2) form (csrc/winograd_ops.hip: wdec_input_kernel, the nine ragged GEMM
    phases of conv_desc_wdec_gemm, wdec_output_item; the packer pack_wdec) through vstab_deconv4x4_winograd, with the tile shape, the
    channel counts and the geometry set by the test: every Ho mod 4 per axis, grids clipped by NT and by the input, pad channels, channel
    slices, both GEMM tiles, the inverse transform alone and riding in the flow head's launch;
  * the flow head predict_up_body (csrc/flow_ops.hip) through vstab_predict_up: both tile sizes, sizes that are no multiple of the tile,
    both output crops, with and without the coarser flow, split-K slab counts around the loop unrolled by four.

Every output buffer starts as a sentinel bit pattern and must keep it outside what the call owns; the workspace and the unread parts of
the inputs hold NaN.  Each comparison prints its largest error as a fraction of its bound (pytest -s; profiles/README.md lists them)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, training
from tests import refine_level_ref as ref

pytestmark = pytest.mark.gpu
SENTINEL = 0x4B1D5EED            # as int32; a finite float
EPS32 = 1.1920929e-07
U32 = 2.0 ** -24                 # unit roundoff of fp32
NAN = float("nan")


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)


def _is_sentinel(t):
    return bool((t.contiguous().view(torch.int32) == SENTINEL).all())


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _fp(a):
    return a.ctypes.data_as(_lib.c_float_p)


# ----------------------------------------------------------------------------- the transposed convolution in Winograd form
def _pack(W, cin, cs_in, cout):
    Wn = np.ascontiguousarray(W.numpy(), np.float32)
    n = 9 * -(-cs_in // 32) * 4 * cout * 32
    wpk = np.empty(n, np.float32)
    assert _lib.lib().vstab_host_pack_wdec_shape(_fp(Wn), None, cin, cs_in, cout, _fp(wpk), n) == n
    return torch.from_numpy(wpk).cuda()


class _Deconv:
    """one problem, drawn once: x [B,Hi,Wi,cs_in] (pad channels zero), W [4,4,cout,cin], bias; nothing here is modified by a test"""

    def __init__(self, B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, act, c_off):
        self.dims = (B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, act, c_off)
        self.cs_out = cout + 16                                               # the slice, 8 floats before or 16 after it
        g = torch.Generator().manual_seed(Hi * 1009 + Ho * 101 + Wi * 53 + Wo * 7 + cs_in + cout + tile)
        self.x = torch.randn(B, Hi, Wi, cs_in, generator=g)
        self.x[..., cin:] = 0.0
        self.W = torch.randn(4, 4, cout, cin, generator=g) / (4 * cin) ** 0.5
        self.bias = torch.randn(cout, generator=g)
        self.junk = torch.randn(B, Hi, Wi, cs_in - cin, generator=g) * 3.0 if cs_in > cin else None
        self.xd, self.bd, self.wpk = self.x.cuda(), self.bias.cuda(), _pack(self.W, cin, cs_in, cout)
        self.ref = ref.deconv_ref(self.x, self.W, self.bias, act, (Ho, Wo))
        self.raw = ref.deconv_ref(self.x, self.W, None, 0, (Ho, Wo))           # before bias and activation
        self.geom = ref.wdec_geom(Hi, Wi, Ho, Wo)

    def run(self, x=None, bias=None, act=None, head=None, out=None):
        """one call on a NaN-filled workspace and a sentinel-filled out; returns (out, the workspace as floats)"""
        B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, act0, c_off = self.dims
        L = _lib.lib()
        nb = L.vstab_deconv4x4_winograd_workspace_bytes(B, Hi, Wi, cs_in, Ho, Wo, cout)
        assert nb > 0 and nb % 256 == 0
        ws = torch.full((nb // 4,), NAN, device="cuda")
        out = _sentinel(B, Ho, Wo, self.cs_out) if out is None else out
        _lib.check(L.vstab_deconv4x4_winograd((self.xd if x is None else x).data_ptr(), B, Hi, Wi, cs_in, self.wpk.data_ptr(),
                                              (self.bd if bias is None else bias).data_ptr(), act0 if act is None else act, out.data_ptr(),
                                              Ho, Wo, self.cs_out, c_off, cout, tile, head, ws.data_ptr(), nb, None))
        torch.cuda.synchronize()
        return out, ws

    def check_against_reference(self, out, what):
        B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, act, c_off = self.dims
        got = out[..., c_off:c_off + cout].double().cpu()
        err = float((got - self.ref).abs().max())                             # (torch's max hands a NaN on)
        tol = 2e-5 * float(self.ref.abs().max()) + 1e-6
        print(f"wdec {what} {self.dims}: max|ref| {float(self.ref.abs().max()):.3f} err {err:.3e} tol {tol:.3e} ({err / tol:.3f})")
        assert err <= tol, (err, tol)
        assert _is_sentinel(out[..., :c_off]) and _is_sentinel(out[..., c_off + cout:])


AXIS = [(Hi, Ho) for Hi in range(1, 7) for Ho in (2 * Hi - 1, 2 * Hi)]       # every Ho mod 4; (4, 7), (6, 11): clipped by NT; (2, 4): by the input
PAIRS = [(AXIS[k], AXIS[(5 * k + 7) % 12]) for k in range(12)] + [((4, 7), (4, 7)), ((2, 4), (6, 11))]
CHANNELS = [(32, 32), (34, 36), (68, 68)]                                      # (cin, cs_in)
COUTS = [32, 64]
DECONV_CASES = []
for k, ((Hi, Ho), (Wi, Wo)) in enumerate(PAIRS):
    for tile in (0, 1):
        DECONV_CASES.append((2, Hi, Ho, Wi, Wo) + CHANNELS[k % 3] + (COUTS[k % 2], tile, (k + tile) % 2, 8 * ((k // 2 + tile) % 2)))
# 3 x 7 x 10 = 210 GEMM rows in position (0, 0): across a 128-row tile and the 256-item workgroups of both transforms
for k, (B, Hi, Ho, Wi, Wo) in enumerate([(3, 13, 25, 18, 36), (3, 13, 26, 18, 35)]):
    for j, ((cin, cs_in), cout, tile) in enumerate(itertools.product(CHANNELS, COUTS, (0, 1))):
        DECONV_CASES.append((B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, (j + k) % 2, 8 * ((j // 2 + k) % 2)))


def _deconv_id(c):
    return "B%d-h%dto%d-w%dto%d-c%dof%d-o%d-tile%d-act%d-off%d" % c


@pytest.fixture(scope="module", params=DECONV_CASES, ids=_deconv_id)
def deconv(request):
    c = _Deconv(*request.param)
    c.out, c.ws = c.run()
    yield c
    del c


def test_case_table_covers_what_it_claims():
    assert {c[2] % 4 for c in DECONV_CASES} == {0, 1, 2, 3} == {c[4] % 4 for c in DECONV_CASES}
    assert {(c[1], c[2]) for c in DECONV_CASES} >= set(AXIS) and {(c[3], c[4]) for c in DECONV_CASES} >= set(AXIS)
    assert {c[5:8] for c in DECONV_CASES} == {ch + (co,) for ch in CHANNELS for co in COUTS}
    for field in (8, 9, 10):
        assert len({c[field] for c in DECONV_CASES}) == 2
    g = ref.wdec_geom(13, 18, 25, 36)
    assert 3 * g["nty"][0] * g["ntx"][0] == 210


def test_winograd_deconv_vs_fp64_reference(deconv):
    """the slice against conv_transpose2d in float64 (+ bias, leaky relu): 2e-5 max|ref| + 1e-6, tests/test_gpu_kloop.py's bound for this
    MFMA kernel family (the direct form meets it); the other channels of out keep the sentinel; the workspace was NaN, so a plane the
    input transform leaves unwritten that reached the result would show as NaN"""
    deconv.check_against_reference(deconv.out, "alone")


def test_transforms_write_exactly_the_tiles_the_gemm_reads(deconv):
    """the workspace starts with V [B][9][NTy][NTx][cs_in], then (256-byte aligned) M [B][9][NTy][NTx][4 cout] (vstab.h): position (i, j)
    holds numbers for the tiles ty < nty[i], tx < ntx[j] and is left as it was -- NaN here -- everywhere else, in both"""
    B, Hi, Ho, Wi, Wo, cin, cs_in, cout = deconv.dims[:8]
    g = deconv.geom
    planes = B * 9 * g["NTy"] * g["NTx"]
    v_floats = -(-planes * cs_in * 4 // 256) * 64
    V = deconv.ws[:planes * cs_in].view(B, 3, 3, g["NTy"], g["NTx"], cs_in).cpu()
    M = deconv.ws[v_floats:v_floats + planes * 4 * cout].view(B, 3, 3, g["NTy"], g["NTx"], 4 * cout).cpu()
    for i in range(3):
        for j in range(3):
            for T in (V, M):
                written = ~torch.isnan(T[:, i, j])
                assert bool(written[:, :g["nty"][i], :g["ntx"][j]].all()), (i, j)
                assert not bool(written[:, g["nty"][i]:].any()) and not bool(written[:, :, g["ntx"][j]:].any()), (i, j)


def test_pad_channels_of_x_change_nothing(deconv):
    """finite non-zero numbers in channels cin .. cs_in of every pixel meet zero rows of the operand: the same bits (a pixel without
    pad channels: a second run on a fresh workspace gives the same bits)"""
    cin = deconv.dims[5]
    x = deconv.x.clone()
    if deconv.junk is not None:
        x[..., cin:] = deconv.junk
        assert float(x[..., cin:].abs().min()) > 0.0
    out, _ = deconv.run(x=x.cuda())
    assert _same_bits(out, deconv.out)


def test_winograd_deconv_vs_direct_form(deconv):
    """the same inputs through the direct form (training.conv_dgrad: four sub-pixel phases on the same MFMA kernel), before bias and
    activation: 64 fp32 epsilons of the tensor's magnitude, tests/test_gpu_wdec.py's bound -- the transforms only add and subtract"""
    B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, act, c_off = deconv.dims
    out, _ = deconv.run(bias=torch.zeros(cout, device="cuda"), act=0)
    Wp = torch.zeros(4, 4, cout, cs_in)
    Wp[..., :cin] = deconv.W                                                  # the pad channels of x are zeros and meet zero taps
    direct = training.conv_dgrad(deconv.xd, Wp.cuda(), 2, 1, (Ho, Wo))
    torch.cuda.synchronize()
    mag = max(1.0, float(deconv.raw.abs().max()))
    d = float((out[..., c_off:c_off + cout] - direct).abs().max())
    e = float((direct.double().cpu() - deconv.raw).abs().max())
    print(f"wdec vs direct {deconv.dims}: diff {d:.3e} bound {64 * EPS32 * mag:.3e} ({d / (64 * EPS32 * mag):.3f}); direct vs ref {e:.3e}")
    assert d <= 64 * EPS32 * mag, (d, mag)
    assert e <= 2e-5 * float(deconv.raw.abs().max()) + 1e-6


# ----------------------------------------------------------------------------- the flow head
class _Head:
    """one flow-head problem: `ks` slabs of a tap table `slab_stride` floats apart in a NaN buffer (columns 18..31 NaN too), bias, optional
    coarser flow, upsample filter; concat [B,oh,ow,Cs] with the flow slot at c_off"""

    def __init__(self, B, h, w, ks, oh, ow, with_prev, Cs, c_off, seed=0):
        self.dims = (B, h, w, ks, oh, ow, with_prev, Cs, c_off)
        g = torch.Generator().manual_seed(h * 977 + w * 31 + ks * 7 + oh + ow + int(with_prev) + seed)
        table = B * h * w * 32
        self.slab_stride = table + 64                                          # larger than one table
        buf = torch.full(((ks - 1) * self.slab_stride + table,), NAN)
        self.slabs = torch.full((ks, B, h, w, 32), NAN)
        self.slabs[..., :18] = torch.randn(ks, B, h, w, 18, generator=g)
        for k in range(ks):
            buf[k * self.slab_stride:k * self.slab_stride + table] = self.slabs[k].reshape(-1)
        self.taps = buf.cuda()
        self.bias2 = torch.randn(2, generator=g)
        self.ph, self.pw = (h + 1) // 2, (w + 1) // 2
        self.prev = torch.randn(B, self.ph, self.pw, 2, generator=g) * 2.0 if with_prev else None
        self.up_w = np.ascontiguousarray((torch.randn(64, generator=g) * 0.3).numpy())
        self.up_b = np.ascontiguousarray(torch.randn(2, generator=g).numpy())
        self.bias2_d = self.bias2.cuda()
        self.prev_d = self.prev.cuda() if with_prev else None

    def buffers(self):
        B, h, w, ks, oh, ow, with_prev, Cs, c_off = self.dims
        return _sentinel(B, h, w, 2), _sentinel(B, oh, ow, Cs)

    def args(self, out, concat, Cs=None, c_off=None):
        """the arguments after B of vstab_predict_up as a vstab_predict_up_args (the arrays it points to live in self)"""
        B, h, w, ks, oh, ow, with_prev, Cs0, c_off0 = self.dims
        return _lib.PredictUpArgs(self.taps.data_ptr(), ks, self.slab_stride, h, w, self.bias2_d.data_ptr(),
                                  self.prev_d.data_ptr() if with_prev else None, self.ph if with_prev else 0, self.pw if with_prev else 0,
                                  out.data_ptr(), _fp(self.up_w), _fp(self.up_b), concat.data_ptr(), oh, ow, Cs0 if Cs is None else Cs,
                                  c_off0 if c_off is None else c_off)

    def run(self):
        out, concat = self.buffers()
        a = self.args(out, concat)
        _lib.check(_lib.lib().vstab_predict_up(a.taps, a.ks, a.slab_stride, self.dims[0], a.h, a.w, a.bias2, a.prev, a.ph, a.pw, a.out, a.up_w,
                                               a.up_b, a.concat, a.oh, a.ow, a.Cs, a.c_off, None))
        torch.cuda.synchronize()
        return out, concat

    def check(self, out, concat, stats):
        """Flow: per element |got - ref| <= (n + 8) 2^-24 S.  The flow is a sum of n addends (the bias, ks slab entries per in-image tap,
        u twice) whose magnitudes sum to S: any order of fp32 additions is off by at most (n - 1) u S to first order (recursive
        summation, u = 2^-24; stages A and B add slab by slab, then tap by tap).  u itself comes from lerp2, tl + (tr - tl) tx twice and
        top + (bot - top) ty: six roundings on the longest path, each relative to an intermediate that the same expression on
        magnitudes bounds -- that expression is u's share of S; the coordinates are the kernel's own fp32 ones, so they add nothing.
        n - 1 + 6 <= n + 8.  Stage C: against the reference applied to the kernel's own stored flow: eight fused multiply-adds on
        |b| + sum |f w|: 9 2^-24 of that."""
        B, h, w, ks, oh, ow, with_prev, Cs, c_off = self.dims
        r = ref.predict_up_ref(self.slabs, self.bias2, self.prev, self.up_w, self.up_b, (oh, ow))
        got = out.double().cpu()
        err = (got - r["flow"]).abs()
        tol = (r["n"].double() + 8.0) * U32 * r["S"]
        ratio = float((err / tol).max())
        stats["flow"] = max(stats.get("flow", 0.0), ratio)
        assert not bool(torch.isnan(got).any()) and bool((err <= tol).all()), (self.dims, ratio)
        up, mag = ref.upsample_ref(got, self.up_w, self.up_b, (oh, ow))
        slot = concat[..., c_off:c_off + 4].cpu()
        err_c = (slot[..., :2].double() - up).abs()
        tol_c = 9.0 * U32 * mag
        ratio_c = float((err_c / tol_c).max())
        stats["up"] = max(stats.get("up", 0.0), ratio_c)
        assert bool((err_c <= tol_c).all()), (self.dims, ratio_c)
        assert float((slot[..., :2].double() - r["up"]).abs().max()) <= 1e-4 * max(1.0, float(r["up"].abs().max()))      # and the whole chain
        assert bool((slot[..., 2:].view(torch.int32) == 0).all())             # floats 2 and 3 are +0.0 exactly
        assert _is_sentinel(concat[..., :c_off]) and _is_sentinel(concat[..., c_off + 4:])


SLOTS = [(4, 0), (20, 0), (20, 8)]                                             # (Cs, c_off)


@pytest.mark.parametrize("ks", [1, 2, 4, 5, 7])
@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (2, 3), (5, 9), (11, 13), (17, 33)])
def test_flow_head_vs_fp64_reference(h, w, ks):
    """sizes that are no multiple of the 4 x 4 tile (one tile, several, a ragged last one), both output crops per axis, without and with
    the coarser flow of (ceil(h/2), ceil(w/2)) -- h = 11 from 6: a scale that is inexact in binary --, slab counts around the loop
    unrolled by four; two different samples"""
    stats = {}
    for idx, (oh, ow, with_prev) in enumerate(itertools.product((2 * h - 1, 2 * h), (2 * w - 1, 2 * w), (False, True))):
        Cs, c_off = SLOTS[(idx + ks) % 3]
        hd = _Head(2, h, w, ks, oh, ow, with_prev, Cs, c_off)
        hd.check(*hd.run(), stats)
    print(f"predict_up {h}x{w} ks={ks}: largest error / bound: flow {stats['flow']:.3f}, upsample {stats['up']:.3f}")


@pytest.mark.parametrize("B,T", [(4, 8), (3, 4)])
def test_flow_head_both_tile_sizes_at_64x64(B, T):
    """B = 4 of 64 x 64 is 256 tiles of 8 x 8: predict_up_kernel<8>; B = 3 stays below and runs <4> (launch_predict_up's rule)"""
    assert (8 if ((64 + 7) // 8) * ((64 + 7) // 8) * B >= 256 else 4) == T
    stats = {}
    for oh, ow, with_prev, ks, (Cs, c_off) in ((128, 127, True, 5, SLOTS[2]), (127, 128, False, 2, SLOTS[0])):
        hd = _Head(B, 64, 64, ks, oh, ow, with_prev, Cs, c_off)
        hd.check(*hd.run(), stats)
    print(f"predict_up B={B} 64x64 (tile {T}): largest error / bound: flow {stats['flow']:.3f}, upsample {stats['up']:.3f}")


def test_flow_head_refusals():
    """each returns its error without a launch: the buffers keep the sentinel"""
    hd = _Head(2, 5, 9, 2, 10, 17, True, 20, 8)
    out, concat = hd.buffers()
    L = _lib.lib()

    def call(**kw):
        a = hd.args(out, concat)
        B = kw.pop("B", 2)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.vstab_predict_up(a.taps, a.ks, a.slab_stride, B, a.h, a.w, a.bias2, a.prev, a.ph, a.pw, a.out, a.up_w, a.up_b, a.concat,
                                  a.oh, a.ow, a.Cs, a.c_off, None)

    assert call(Cs=18) == -1 and call(Cs=8, c_off=8) == -1 and call(c_off=20) == -1 and call(c_off=6) == -1 and call(ks=0) == -1
    assert call(oh=11) == -1 and call(ow=19) == -1 and call(B=0) == -1 and call(h=0) == -1 and call(ph=0) == -1
    assert call(slab_stride=hd.slab_stride - 1) == -1 and call(slab_stride=64) == -1
    for name in ("taps", "bias2", "out", "concat"):
        assert call(**{name: None}) == -6, name
    assert call(up_w=None) == -6 and call(up_b=None) == -6
    assert call(taps=hd.taps.data_ptr() + 4) == -2 and call(out=out.data_ptr() + 4) == -2 and call(concat=concat.data_ptr() + 8) == -2
    assert call(prev=hd.prev_d.data_ptr() + 4) == -2
    torch.cuda.synchronize()
    assert _is_sentinel(out) and _is_sentinel(concat)
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out.view(torch.int32) == SENTINEL).any())


# ----------------------------------------------------------------------------- the inverse transform riding in the flow head's launch
@pytest.mark.parametrize("B,Hi,Ho,Wi,Wo,cin,cs_in,cout,tile,act,c_off,with_prev,ks", [
    (2, 1, 2, 1, 1, 32, 32, 32, 0, 1, 0, False, 1),
    (2, 5, 10, 9, 17, 34, 36, 64, 1, 1, 8, True, 5),
    (3, 13, 25, 18, 36, 68, 68, 32, 0, 0, 0, True, 2),
    (3, 13, 26, 18, 35, 32, 32, 64, 1, 1, 8, False, 4),
    (4, 64, 128, 64, 127, 32, 32, 32, 0, 1, 8, True, 2),                       # 256 head tiles: wdec_output_predict_up_kernel<8>
], ids=lambda v: str(v))
def test_inverse_transform_in_the_flow_heads_launch(B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, act, c_off, with_prev, ks):
    """as in the forward: the head reads the level's tap table and writes its flow and, into the SAME concat buffer as the transposed
    convolution's slice, the upsampled flow.  The slice is the head = NULL call's bit for bit (and meets the reference); the flow and the
    upsampled slot are vstab_predict_up's bit for bit (and meet its reference); everything else keeps the sentinel"""
    dc = _Deconv(B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, act, c_off)
    alone, _ = dc.run()
    dc.check_against_reference(alone, "alone")
    slot = dc.cs_out - 4 if c_off == 0 else 0                                 # the flow's four floats: after / before the slice
    hd = _Head(B, Hi, Wi, ks, Ho, Wo, with_prev, dc.cs_out, slot, seed=1)
    flow_alone, concat_alone = hd.run()
    hd.check(flow_alone, concat_alone, {})
    flow = _sentinel(B, Hi, Wi, 2)
    out = _sentinel(B, Ho, Wo, dc.cs_out)
    a = hd.args(flow, out)
    fused, _ = dc.run(head=C.byref(a), out=out)
    assert _same_bits(fused[..., c_off:c_off + cout], alone[..., c_off:c_off + cout])
    assert _same_bits(flow, flow_alone)
    assert _same_bits(fused[..., slot:slot + 4], concat_alone[..., slot:slot + 4])
    owned = torch.zeros(dc.cs_out, dtype=torch.bool)
    owned[c_off:c_off + cout] = True
    owned[slot:slot + 4] = True
    assert _is_sentinel(fused[..., (~owned).cuda()])
    # a head the flow head itself refuses is refused here too, before anything is launched
    out2 = _sentinel(B, Ho, Wo, dc.cs_out)
    bad = hd.args(flow, out2, c_off=dc.cs_out)
    B_, nb = dc.dims[0], _lib.lib().vstab_deconv4x4_winograd_workspace_bytes(B, Hi, Wi, cs_in, Ho, Wo, cout)
    ws = torch.full((nb // 4,), NAN, device="cuda")
    assert _lib.lib().vstab_deconv4x4_winograd(dc.xd.data_ptr(), B_, Hi, Wi, cs_in, dc.wpk.data_ptr(), dc.bd.data_ptr(), act, out2.data_ptr(), Ho, Wo,
                                               dc.cs_out, c_off, cout, tile, C.byref(bad), ws.data_ptr(), nb, None) == -1
    torch.cuda.synchronize()
    assert _is_sentinel(out2) and bool(torch.isnan(ws).all())


def test_winograd_deconv_refusals():
    """what wdec_applies and the launchers refuse, with the usual codes and without a launch"""
    dc = _Deconv(2, 5, 10, 9, 17, 34, 36, 64, 0, 1, 8)
    B, Hi, Ho, Wi, Wo, cin, cs_in, cout, tile, act, c_off = dc.dims
    L = _lib.lib()
    nb = L.vstab_deconv4x4_winograd_workspace_bytes(B, Hi, Wi, cs_in, Ho, Wo, cout)
    ws = torch.full((nb // 4 + 64,), NAN, device="cuda")
    out = _sentinel(B, Ho, Wo, dc.cs_out)
    base = dict(x=dc.xd.data_ptr(), B=B, Hi=Hi, Wi=Wi, cs_in=cs_in, wpk=dc.wpk.data_ptr(), bias=dc.bd.data_ptr(), act=act, out=out.data_ptr(),
                Ho=Ho, Wo=Wo, cs_out=dc.cs_out, c_off=c_off, cout=cout, tile=tile, head=None, ws=ws.data_ptr(), nb=nb, stream=None)

    def call(**kw):
        return L.vstab_deconv4x4_winograd(*{**base, **kw}.values())

    for bad in (dict(cs_in=34), dict(cout=48), dict(cout=16), dict(cout=544), dict(Ho=8), dict(Ho=11), dict(Wo=16), dict(Wo=19), dict(tile=2), dict(tile=3),
                dict(act=2), dict(cs_out=82), dict(c_off=6), dict(c_off=20), dict(B=0), dict(Hi=0)):
        assert call(**bad) == -1, bad
    assert call(B=4096, Hi=256, Ho=512, Wi=256, Wo=512) == -1                 # tensors of 2 GiB and more
    assert L.vstab_deconv4x4_winograd_workspace_bytes(4096, 256, 256, cs_in, 512, 512, cout) == 0
    assert L.vstab_deconv4x4_winograd_workspace_bytes(B, Hi, Wi, 34, Ho, Wo, cout) == 0
    assert L.vstab_deconv4x4_winograd_workspace_bytes(B, Hi, Wi, cs_in, Ho + 1, Wo, cout) == 0
    for name in ("x", "wpk", "bias", "out", "ws"):
        assert call(**{name: None}) == -6, name
        assert call(**{name: base[name] + (16 if name == "ws" else 4)}) == -2, name
    assert call(nb=nb - 1) == -4
    torch.cuda.synchronize()
    assert _is_sentinel(out) and bool(torch.isnan(ws).all())
    assert call() == 0
    torch.cuda.synchronize()
    dc.check_against_reference(out, "after the refusals")
