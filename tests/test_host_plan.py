"""Host logic of libvstab_hip.so checked on the CPU: the forward schedule's per-layer
GEMM geometry (vstab_host_layer_plan) and the weight packer (vstab_host_pack_layer) are
run through a numpy emulation of what the implicit-GEMM kernel computes
(out[m, n] = sum_k A[m, k] * Wpacked[k, n], A gathered exactly as ConvParams describes)
and compared with the oracle's convolution / transposed convolution."""
import ctypes as C

import numpy as np
import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, netspec
from oracle import vstab_oracle as vo

FIELDS = ("B Hi Wi Cs_in KH NSEG SEG SEGP SEG_STRIDE s_in s_out Ho Wo Cs_out c_off N Npad act nphase ksplit "
          "Mmax tile vec4 in_buf out_buf reserved").split()
PH_FIELDS = "Hg Wg M off_y off_x o_y o_x".split()


def layer_plan(B, H, W, Cin, layer):
    buf = (C.c_int32 * 64)()
    n = _lib.lib().vstab_host_layer_plan(B, H, W, Cin, layer, buf, 64)
    assert n > 0
    p = dict(zip(FIELDS, buf[:26]))
    p["ph"] = [dict(zip(PH_FIELDS, buf[26 + 7 * k:33 + 7 * k])) for k in range(p["nphase"])]
    return p


def pack_layer(Cin, layer, W, scale=None):
    W = np.ascontiguousarray(W, np.float32)
    cap = 64 * 1024 * 1024
    out = np.zeros(cap, np.float32)
    sc = None if scale is None else np.ascontiguousarray(scale, np.float64).ctypes.data_as(C.POINTER(C.c_double))
    n = _lib.lib().vstab_host_pack_layer(Cin, layer, W.ctypes.data_as(_lib.c_float_p), sc,
                                         out.ctypes.data_as(_lib.c_float_p), cap)
    assert n > 0, _lib.lib().vstab_last_error(None)
    return out[:n]


def swz32(n, k):
    return (((k >> 2) ^ ((n >> 1) & 7)) << 2) | (k & 3)


def emulate(inp, p, wpk):
    """inp [B,Hi,Wi,Cs_in] float64 -> out [B,Ho,Wo,Cs_out] float64 (NaN where the layer does not write)."""
    B, Hi, Wi, Cs = p["B"], p["Hi"], p["Wi"], p["Cs_in"]
    KT = p["KH"] * p["NSEG"] * p["SEGP"] // 32
    Np = p["Npad"]
    wpk = wpk.reshape(p["nphase"], KT, Np, 32).astype(np.float64)
    unsw = np.array([[swz32(n, k) for k in range(32)] for n in range(Np)])           # [Np, 32]
    Wm = np.take_along_axis(wpk, np.broadcast_to(unsw, wpk.shape), axis=3)             # logical k order
    Wm = Wm.transpose(0, 1, 3, 2).reshape(p["nphase"], KT * 32, Np)
    rows = inp.reshape(B, Hi, Wi * Cs)
    out = np.full((B, p["Ho"], p["Wo"], p["Cs_out"]), np.nan)
    for k, ph in enumerate(p["ph"]):
        m = np.arange(ph["M"])
        n, rem = np.divmod(m, ph["Hg"] * ph["Wg"])
        j, i = np.divmod(rem, ph["Wg"])
        A = np.zeros((ph["M"], KT * 32))
        for t in range(p["KH"]):
            iy = j * p["s_in"] + ph["off_y"] + t
            yok = (iy >= 0) & (iy < Hi)
            for s in range(p["NSEG"]):
                q = np.arange(p["SEG"])
                foff = ((i * p["s_in"] + ph["off_x"]) * Cs)[:, None] + (s * p["SEG_STRIDE"] + q)[None, :]
                ok = yok[:, None] & (foff >= 0) & (foff < Wi * Cs)
                vals = rows[n[:, None], np.clip(iy, 0, Hi - 1)[:, None], np.clip(foff, 0, Wi * Cs - 1)]
                k0 = (t * p["NSEG"] + s) * p["SEGP"]
                A[:, k0:k0 + p["SEG"]] = np.where(ok, vals, 0.0)
        res = A @ Wm[k]
        out[n, j * p["s_out"] + ph["o_y"], i * p["s_out"] + ph["o_x"], p["c_off"]:p["c_off"] + p["N"]] = res[:, :p["N"]]
    return out


ENC = netspec.ENCODER


@pytest.mark.parametrize("layer", list(range(10)))
@pytest.mark.parametrize("cin", [27, 6])
def test_encoder_layer_geometry_and_packing(layer, cin):
    if cin == 6 and layer > 0:
        pytest.skip("Cin only changes layer 0")
    H, W, B = (52, 44, 2) if layer < 4 else (96, 80, 1)
    p = layer_plan(B, H, W, cin, layer)
    st = ENC[layer]
    ci = cin if layer == 0 else ENC[layer - 1].cout
    rng = np.random.default_rng(layer)
    inp = rng.standard_normal((B, p["Hi"], p["Wi"], p["Cs_in"]))          # pad channels random on purpose
    Wt = rng.standard_normal((st.k, st.k, ci, st.cout)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, p["Npad"])
    got = emulate(inp, p, pack_layer(cin, layer, Wt, scale))
    ref = vo.pad_conv(torch.from_numpy(inp[..., :ci].copy()), torch.from_numpy(Wt.astype(np.float64)), None,
                      st.pad, st.stride).numpy() * scale[:st.cout]
    assert got.shape[1:3] == ref.shape[1:3]
    sl = got[..., p["c_off"]:p["c_off"] + st.cout]
    assert np.abs(sl - ref).max() < 1e-5 * max(1, np.abs(ref).max())    # packed weights are fp32(W*scale)
    assert np.isnan(got[..., st.cout:]).all()                            # nothing written outside the slice


@pytest.mark.parametrize("l", [0, 1, 2, 3])
@pytest.mark.parametrize("HW", [(64, 64), (88, 104)])     # second size has odd output grids
def test_deconv_phase_geometry_and_packing(l, HW):
    H, W = HW
    B = 1
    p = layer_plan(B, H, W, 27, 10 + l)
    cin = (1024, 1026, 770, 386)[l]
    cout = (512, 256, 128, 64)[l]
    rng = np.random.default_rng(10 + l)
    inp = rng.standard_normal((B, p["Hi"], p["Wi"], p["Cs_in"]))
    Wt = (rng.standard_normal((4, 4, cout, cin)) * 0.1).astype(np.float32)
    got = emulate(inp, p, pack_layer(27, 10 + l, Wt))
    ref = vo.deconv4x4s2(torch.from_numpy(inp[..., :cin].copy()), torch.from_numpy(Wt.astype(np.float64)), None,
                         (p["Ho"], p["Wo"])).numpy()
    sl = got[..., p["c_off"]:p["c_off"] + cout]
    assert not np.isnan(sl).any()                                        # the 4 phases cover every output pixel
    assert np.abs(sl - ref).max() < 1e-9 * max(1, np.abs(ref).max())
    assert np.isnan(got[..., :p["c_off"]]).all() and np.isnan(got[..., p["c_off"] + cout:]).all()


def test_predict2_tap_table():
    p = layer_plan(1, 64, 64, 27, 14)
    rng = np.random.default_rng(5)
    inp = rng.standard_normal((1, p["Hi"], p["Wi"], 196))
    Wt = rng.standard_normal((3, 3, 194, 2)).astype(np.float32)
    got = emulate(inp, p, pack_layer(27, 14, Wt))
    ref = np.einsum("bhwc,tco->bhwto", inp[..., :194], Wt.reshape(9, 194, 2).astype(np.float64)).reshape(1, p["Hi"], p["Wi"], 18)
    assert np.abs(got[..., :18] - ref).max() < 1e-9
    assert np.abs(got[..., 18:32]).max() == 0


@pytest.mark.parametrize("layer,cin,cs", [(15, 1024, 1024), (16, 1026, 1028), (17, 770, 772), (18, 386, 388)])
def test_predict_head_tap_tables(layer, cin, cs):
    p = layer_plan(1, 64, 64, 27, layer)
    assert p["Cs_in"] == cs
    rng = np.random.default_rng(layer)
    inp = rng.standard_normal((1, p["Hi"], p["Wi"], cs))
    Wt = rng.standard_normal((3, 3, cin, 2)).astype(np.float32)
    got = emulate(inp, p, pack_layer(27, layer, Wt))
    ref = np.einsum("bhwc,tco->bhwto", inp[..., :cin], Wt.reshape(9, cin, 2).astype(np.float64)).reshape(1, p["Hi"], p["Wi"], 18)
    assert np.abs(got[..., :18] - ref).max() < 1e-9 * max(1, np.abs(ref).max())
    assert np.abs(got[..., 18:32]).max() == 0


def test_split_k_plan_is_consistent():
    for (B, H, W) in ((8, 512, 512), (1, 256, 256), (2, 720, 1280)):
        for layer in range(19):
            p = layer_plan(B, H, W, 27, layer)
            KT = p["KH"] * p["NSEG"] * p["SEGP"] // 32
            kts = -(-KT // p["ksplit"])
            assert (p["ksplit"] - 1) * kts < KT                         # no empty split
            if p["ksplit"] > 1:
                assert p["N"] % 4 == 0 and p["Cs_out"] % 4 == 0 and p["c_off"] % 4 == 0
            if p["vec4"]:
                assert p["Cs_in"] % 4 == 0 and p["SEG"] % 4 == 0 and p["SEG_STRIDE"] % 4 == 0
            # tile ids: 128x128, 128x64, 128x32, 64x128, 64x64 (harness builds only), 256x32, weight-stream kernel (32 columns)
            assert p["tile"] != 4 and p["Npad"] % (128, 64, 32, 128, 64, 32, 32)[p["tile"]] == 0
            if p["tile"] == 6:                                           # few rows per phase, a ticket word per (phase, row tile, column block)
                assert p["Mmax"] <= 64 and -(-p["Mmax"] // 32) * (p["Npad"] // 32) * p["nphase"] <= 4096
                assert p["ksplit"] <= 16


def test_workspace_layout_is_disjoint_and_aligned():
    L = _lib.lib()
    ent = (_lib.VstabWsEntry * 24)()
    n = L.vstab_workspace_layout(8, 512, 512, 27, ent, 24)
    assert n == 19          # 10 activation buffers, 5 tap tables, the ticket words, split-K slabs, the two Winograd-domain buffers
    names = [e.name.decode() for e in ent[:n]]
    assert names[-4:] == ["tickets", "splitk", "winograd_in", "winograd_out"]      # the plan-dependent sizes come last (vstab.h)
    assert ent[n - 4].w == 4096                                                   # one ticket word per (phase, row tile, column block)
    total = L.vstab_workspace_bytes(8, 512, 512, 27)
    spans = []
    for e in ent[:n]:
        assert e.offset_bytes % 256 == 0
        spans.append((e.offset_bytes, e.offset_bytes + 4 * e.n * e.h * e.w * e.c_stride))
    spans.sort()
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0
    assert spans[-1][1] <= total
    assert L.vstab_workspace_bytes(1, 2, 2, 27) == 0                      # too small for the net


def layer_tiles(B, H, W, flags=0, plan_batch=0):
    out = (C.c_int32 * 200)()
    tiles = []
    for layer in range(19):
        n = _lib.lib().vstab_host_layer_plan_pinned(plan_batch, flags, B, H, W, 27, layer, out, 200)
        assert n > 0, (B, H, W, layer)
        tiles.append((out[21], out[19], out[25]))          # tile id, split-K factor, Winograd form
    return tiles


def test_pinned_plan_is_the_plan_of_its_batch():
    # vstab_set_plan_batch: every decision that changes the order of a sample's sums (split-K factor, Winograd or direct form, weight-stream
    # or tiled kernel) of ANY batch up to the pinned one is the pinned batch's own (of one 2 GiB chunk of it: 16 x 1080p runs as 2 x 8)
    for (P, H, W) in ((8, 512, 512), (4, 384, 512), (16, 1080, 1920)):
        rb = 8 if H == 1080 else P
        ref = layer_tiles(rb, H, W)
        for b in (1, 3, rb):
            got = layer_tiles(b, H, W, plan_batch=P)
            assert [(t[1], t[2], t[0] == 6) for t in got] == [(t[1], t[2], t[0] == 6) for t in ref], (P, b)
    assert layer_tiles(1, 512, 512) != layer_tiles(1, 512, 512, plan_batch=8)        # a lone sample plans differently by itself
    out = (C.c_int32 * 200)()
    assert _lib.lib().vstab_host_layer_plan_pinned(4, 0, 5, 384, 512, 27, 3, out, 200) < 0      # beyond the pinned batch
    # flag 1: the round-3 schedule (few-row layers on the tiled kernel with a combine launch)
    assert any(t[0] == 6 for t in layer_tiles(1, 256, 256)) and not any(t[0] == 6 for t in layer_tiles(1, 256, 256, flags=1))


# ---- Winograd F(2x2,2x2) form of the transposed convolutions (round 6; csrc/winograd_ops.hip documents the algebra).  The host side --
# tile geometry, the 9-position GEMM's plan, the packed operands -- is run through the numpy GEMM emulation between numpy statements
# of the two transforms (the device kernels' arithmetic, statement for statement) and compared with the oracle's transposed convolution.
def wdec_plan(B, H, W, l):
    buf = (C.c_int32 * 128)()
    n = _lib.lib().vstab_host_wdec_plan(B, H, W, 27, l, buf, 128)
    assert n == 26 + 63 + 8
    p = dict(zip(FIELDS, buf[:26]))
    p["ph"] = [dict(zip(PH_FIELDS, buf[26 + 7 * k:33 + 7 * k])) for k in range(9)]
    g = list(buf[89:97])
    return p, dict(NTy=g[0], NTx=g[1], nty=g[2:5], ntx=g[5:8])


def wdec_input_np(x, g):
    """x [B,Hi,Wi,Cs] -> V [B, 9*NTy, NTx, Cs]; tiles a position does not need stay NaN (the GEMM must not read them)."""
    B, Hi, Wi, Cs = x.shape
    xp = np.zeros((B, 2 * g["NTy"] + 2, 2 * g["NTx"] + 2, Cs))
    xp[:, 1:1 + Hi, 1:1 + Wi] = x                                   # xp[r] = x[r - 1]: tile t reads rows 2t-1 .. 2t+1 = xp[2t .. 2t+2]
    V = np.full((B, 9 * g["NTy"], g["NTx"], Cs), np.nan)
    d = [[xp[:, i:i + 2 * g["NTy"]:2, j:j + 2 * g["NTx"]:2] for j in range(3)] for i in range(3)]
    t = [[d[0][j] - d[1][j] for j in range(3)], [d[1][j] for j in range(3)], [d[1][j] - d[2][j] for j in range(3)]]
    for i in range(3):
        v = [t[i][0] - t[i][1], t[i][1], t[i][1] - t[i][2]]
        for j in range(3):
            pos = i * 3 + j
            V[:, pos * g["NTy"]:pos * g["NTy"] + g["nty"][i], :g["ntx"][j]] = v[j][:, :g["nty"][i], :g["ntx"][j]]
    return V


def wdec_output_np(M, g, cout, Ho, Wo):
    """M [B, 9*NTy, NTx, 4*cout] (NaN where the GEMM wrote nothing) -> y [B,Ho,Wo,cout]"""
    B = M.shape[0]
    m = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            pos = i * 3 + j
            blk = np.zeros((B, g["NTy"], g["NTx"], 4 * cout))
            blk[:, :g["nty"][i], :g["ntx"][j]] = M[:, pos * g["NTy"]:pos * g["NTy"] + g["nty"][i], :g["ntx"][j]]
            m[i][j] = blk
    y = np.full((B, Ho, Wo, cout), np.nan)
    s = [[m[0][j] + m[1][j] for j in range(3)], [m[1][j] - m[2][j] for j in range(3)]]
    for a in range(2):
        for b in range(2):
            blk = s[a][0] + s[a][1] if b == 0 else s[a][1] - s[a][2]
            for py in range(2):
                for px in range(2):
                    for ty in range(g["NTy"]):
                        oy = 4 * ty + 2 * a - py
                        if not 0 <= oy < Ho:
                            continue
                        ox = 4 * np.arange(g["NTx"]) + 2 * b - px
                        ok = (ox >= 0) & (ox < Wo)
                        ph = 2 * py + px
                        y[:, oy, ox[ok]] = blk[:, ty, ok, ph * cout:(ph + 1) * cout]
    return y


@pytest.mark.parametrize("l", [1, 2, 3])
@pytest.mark.parametrize("HW", [(64, 64), (88, 104), (96, 128)])     # (88, 104): odd output grids on some levels
def test_winograd_deconv_geometry_packing_and_transforms(l, HW):
    H, W = HW
    B = 2
    d = layer_plan(B, H, W, 27, 10 + l)                               # the direct form: sizes and channel strides
    p, g = wdec_plan(B, H, W, l)
    cin = (1024, 1026, 770, 386)[l]
    cout = (512, 256, 128, 64)[l]
    assert p["N"] == 4 * cout and p["nphase"] == 9 and p["Cs_in"] == d["Cs_in"] and p["ksplit"] == 1
    assert g["NTy"] == d["Ho"] // 4 + 1 and g["NTx"] == d["Wo"] // 4 + 1
    rng = np.random.default_rng(20 + l)
    inp = rng.standard_normal((B, d["Hi"], d["Wi"], d["Cs_in"]))
    inp[..., cin:] = 0.0                                              # the concat's pad channels are zeros (and meet zero weights)
    Wt = (rng.standard_normal((4, 4, cout, cin)) * 0.1).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout)
    cap = 9 * (p["SEGP"] // 32) * 4 * cout * 32
    wpk = np.zeros(cap, np.float32)
    n = _lib.lib().vstab_host_pack_wdec(l, Wt.ctypes.data_as(_lib.c_float_p), scale.ctypes.data_as(C.POINTER(C.c_double)),
                                        wpk.ctypes.data_as(_lib.c_float_p), cap)
    assert n == cap
    V = wdec_input_np(inp, g)
    assert p["Hi"] == V.shape[1] and p["Wi"] == V.shape[2]
    Vz = np.where(np.isnan(V), 1e30, V)                               # a tile the GEMM should skip would blow the result up
    M = emulate(Vz, p, wpk)
    got = wdec_output_np(M, g, cout, d["Ho"], d["Wo"])
    ref = vo.deconv4x4s2(torch.from_numpy(inp[..., :cin].copy()), torch.from_numpy(Wt.astype(np.float64)), None,
                         (d["Ho"], d["Wo"])).numpy() * scale
    assert not np.isnan(got).any()                                    # every output pixel is produced
    assert np.abs(got - ref).max() < 2e-6 * max(1, np.abs(ref).max())       # operands are fp32(G g G^T * scale)
    # multiply-adds per output channel and input channel: one per GEMM row and phase column against four taps per output pixel, direct
    issued = sum(ph["M"] for ph in p["ph"]) * 4
    direct = B * d["Ho"] * d["Wo"] * 4
    assert issued / direct >= 9 / 16                                  # 9 multiplies per 4x4 outputs x 4 ... / 64, plus the ragged grid
    if min(d["Hi"], d["Wi"]) >= 12:
        assert issued / direct < 0.75, issued / direct


# ---- the stream form of a Winograd stage's 16 GEMMs (csrc/wino_gemm_stream.hip): the launcher's rule, and the layout of the operand that
# tests/test_gpu_wino_gemm_stream.py hands both forms of the GEMM
def stream_positions(B, T, cin, cout):
    return _lib.lib().vstab_host_wino_stream_positions(B, T, cin, cout)


# B, T, cin, cout, positions per workgroup: B * (T/128) * (cout/64) * (16/P) == 512 workgroups each (the cases of the GPU test)
STREAM_CASES = [
    (8, 1024, 256, 256, 8),        # conv3_1 at B=8 512x512
    (8, 256, 512, 512, 4),         # conv4_1 at B=8 512x512
    (4, 256, 512, 512, 2),         # conv4_1 at B=4: two row tiles per sample
    (8, 1024, 128, 512, 16),       # one workgroup owns all 16 positions; four K-tiles per position: one pair of loop bodies
    (2, 4096, 128, 64, 2),         # a single column tile
    (1, 1024, 192, 512, 2),        # one sample; six K-tiles per position
    (8, 128, 1024, 512, 2),        # one row tile per sample: sample index = tile index; 32 K-tiles per position
]


def test_wino_stream_positions_rule():
    # the network's two streamed stages (conv3_1: 32x32 tiles of 256 -> 256 channels, conv4_1: 16x16 tiles of 512 -> 512) at 512x512
    for B, p3, p4 in ((4, 4, 2), (8, 8, 4), (16, 16, 8)):
        assert stream_positions(B, 1024, 256, 256) == p3 and stream_positions(B, 256, 512, 512) == p4, B
    for B, T, cin, cout, P in STREAM_CASES:
        assert B * (T // 128) * (cout // 64) * (16 // P) == 512
        assert stream_positions(B, T, cin, cout) == P, (B, T, cin, cout)
    # each of these breaks one condition; with that condition dropped the tile count would still lead to 512 workgroups for some P
    assert stream_positions(64, 64, 256, 512) == 0           # T below a row tile
    assert stream_positions(8, 192, 512, 512) == 0           # T not whole row tiles
    assert stream_positions(8, 1024, 64, 256) == 0           # two K-tiles per position: below the loop's shortest stream
    assert stream_positions(8, 1024, 160, 256) == 0          # an odd number of K-tiles
    assert stream_positions(8, 1024, 256, 96) == 0           # cout not whole column tiles
    # tiles per position that no P in {2, 4, 8, 16} brings to 512 workgroups
    assert 25 * (512 // 128) * (64 // 64) == 100 and stream_positions(25, 512, 128, 64) == 0
    assert 16 * (1024 // 128) * (512 // 64) == 1024 and stream_positions(16, 1024, 256, 512) == 0


def blocked_pack_np(U):
    """[K][N] row-major -> the MFMA kernels' operand [K/32][N][32]: K-tile kt, column n holds U[32 kt .. 32 kt + 31][n], its 16-byte chunks
    XOR-swizzled by (n >> 1) & 7 (pack.cpp's layout, restated)"""
    K, N = U.shape
    assert K % 32 == 0
    pos = np.array([[swz32(n, k) for k in range(32)] for n in range(N)])                     # [N, 32]: where logical k sits
    out = np.empty((K // 32, N, 32), U.dtype)
    np.put_along_axis(out, np.broadcast_to(pos, out.shape), U.reshape(K // 32, 32, N).transpose(0, 2, 1), axis=2)
    return out


def test_winograd_operand_layout_is_the_blocked_layout_per_position():
    # what vstab_load_weights packs for a Winograd stage (pack_winograd) is, position by position, blocked_pack_np of U[xi] = G g G^T:
    # the layout the GPU test checks the device-side packing of vstab_wino_domain_gemm against.  Integer filters: G g G^T is exact
    # (multiples of 1/4), so the comparison is bit for bit; the scale is folded in double and rounded once on both sides.
    cin, cout = 96, 128
    rng = np.random.default_rng(7)
    Wt = rng.integers(-4, 5, (3, 3, cin, cout)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout)
    G = np.array([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]])
    U = np.einsum("ia,jb,abkn->ijkn", G, G, Wt.astype(np.float64)).reshape(16, cin, cout)
    n = 16 * cin * cout
    for sc in (None, scale):
        wpk = np.full(n + 32, np.nan, np.float32)
        got = _lib.lib().vstab_host_pack_winograd(Wt.ctypes.data_as(_lib.c_float_p),
                                                  None if sc is None else sc.ctypes.data_as(C.POINTER(C.c_double)), cin, cout,
                                                  wpk.ctypes.data_as(_lib.c_float_p), n)
        assert got == n and np.isnan(wpk[n:]).all()
        want = U if sc is None else U * sc
        for xi in range(16):
            assert np.array_equal(wpk[xi * cin * cout:(xi + 1) * cin * cout].reshape(cin // 32, cout, 32),
                                  blocked_pack_np(want[xi].astype(np.float32))), xi
    assert _lib.lib().vstab_host_pack_winograd(Wt.ctypes.data_as(_lib.c_float_p), None, cin, cout, wpk.ctypes.data_as(_lib.c_float_p), n - 1) == -4
    assert _lib.lib().vstab_host_pack_winograd(None, None, cin, cout, wpk.ctypes.data_as(_lib.c_float_p), n) == -1


def wdec_operand_np(Wt, scale, cs_in):
    """U[pos = 3 i + j][ci][ph * cout + co] = (G g G^T)[i][j] * scale[co] in float64, g[a][b] = W[3 - py - 2 a][3 - px - 2 b][co][ci] the
    2 x 2 taps of output phase ph = 2 py + px, G = [1 0; 1 1; 0 1]; rows cin .. round_up(cs_in, 32) are zeros (pack.cpp: pack_wdec)"""
    cout, cin = Wt.shape[2], Wt.shape[3]
    G = np.array([[1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    U = np.zeros((9, -(-cs_in // 32) * 32, 4 * cout))
    for py in range(2):
        for px in range(2):
            g = Wt.astype(np.float64)[3 - py::-2, 3 - px::-2]                # [a][b][co][ci]
            u = np.einsum("ia,jb,aboc->ijco", G, G, g).reshape(9, cin, cout)
            ph = 2 * py + px
            U[:, :cin, ph * cout:(ph + 1) * cout] = u if scale is None else u * scale
    return U


def pack_wdec_shape(Wt, scale, cin, cs_in, cout, cap=None, slack=32):
    n = 9 * -(-cs_in // 32) * 4 * cout * 32
    wpk = np.full(n + slack, np.nan, np.float32)
    got = _lib.lib().vstab_host_pack_wdec_shape(Wt.ctypes.data_as(_lib.c_float_p),
                                                None if scale is None else scale.ctypes.data_as(C.POINTER(C.c_double)), cin, cs_in, cout,
                                                wpk.ctypes.data_as(_lib.c_float_p), n if cap is None else cap)
    return got, n, wpk


@pytest.mark.parametrize("cin,cs_in,cout", [(64, 64, 32), (34, 36, 64)])
def test_wdec_operand_for_arbitrary_channel_counts_vs_fp64_transform(cin, cs_in, cout):
    # integer filters: G g G^T is exact, so the comparison is bit for bit; the scale is folded in double and rounded once on both sides
    rng = np.random.default_rng(cin + cout)
    Wt = rng.integers(-4, 5, (4, 4, cout, cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout)
    for sc in (None, scale):
        got, n, wpk = pack_wdec_shape(Wt, sc, cin, cs_in, cout)
        assert got == n and np.isnan(wpk[n:]).all()
        want = wdec_operand_np(Wt, sc, cs_in).astype(np.float32)
        packed = wpk[:n].reshape(9, -1, 4 * cout, 32)
        for pos in range(9):
            assert np.array_equal(packed[pos], blocked_pack_np(want[pos])), pos
        # the rows of the pad channels and of the K-tile's tail are zeros at every position (they meet whatever the pixel holds there)
        unsw = np.array([[swz32(c, k) for k in range(32)] for c in range(4 * cout)])
        logical = np.take_along_axis(packed, np.broadcast_to(unsw, packed.shape), axis=3)          # [9][KT][4 cout][k]
        rows = logical.transpose(0, 1, 3, 2).reshape(9, -1, 4 * cout)
        assert rows.shape[1] == -(-cs_in // 32) * 32 and not rows[:, cin:].any() and rows[:, :cin].any()
    L = _lib.lib()
    assert pack_wdec_shape(Wt, None, cin, cs_in, cout, cap=n - 1)[0] == -4
    assert pack_wdec_shape(Wt, None, cin, cin - 2, cout)[0] == -1 and pack_wdec_shape(Wt, None, 0, cs_in, cout)[0] == -1
    assert L.vstab_host_pack_wdec_shape(None, None, cin, cs_in, cout, wpk.ctypes.data_as(_lib.c_float_p), n) == -1


@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_wdec_level_operand_is_the_shape_form(l):
    cin, cs, cout = ((1024, 1024, 512), (1026, 1028, 256), (770, 772, 128), (386, 388, 64))[l]
    rng = np.random.default_rng(40 + l)
    Wt = rng.standard_normal((4, 4, cout, cin)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout)
    got, n, want = pack_wdec_shape(Wt, scale, cin, cs, cout, slack=0)
    assert got == n
    wpk = np.full(n, np.nan, np.float32)
    assert _lib.lib().vstab_host_pack_wdec(l, Wt.ctypes.data_as(_lib.c_float_p), scale.ctypes.data_as(C.POINTER(C.c_double)),
                                           wpk.ctypes.data_as(_lib.c_float_p), n) == n
    assert np.array_equal(wpk, want)


# ---- how a filter gradient is launched (csrc/wgrad_mfma.hip: wgrad_choose_split; csrc/train_conv_api.cpp: wgrad_split, wino_wgrad_shape), as
# vstab_host_wgrad_split reports it: the cases of tests/test_gpu_wgrad_alone.py, each chosen for what its reduction hits
def wgrad_split(M, cout, K, nbatch=0):
    """(n_main, n_tail, ks_main, ks_tail) of the launches of a reduction over K pixels into M x cout"""
    out = (C.c_int32 * 4)()
    assert _lib.lib().vstab_host_wgrad_split(M, cout, K, nbatch, out) == 0, (M, cout, K, nbatch)
    return tuple(out)


def wgrad_case_K(case):
    B, Hi, Wi, _, _, k, s, p = case
    return B * ((Hi + 2 * p - k) // s + 1) * ((Wi + 2 * p - k) // s + 1)


# (B, Hi, Wi, cin, cout, k, s, p), K = B*Ho*Wo (the symmetric-pad output size), (n_main, n_tail, ks_main, ks_tail)
WGRAD_SPLIT_CASES = [
    ((1, 1, 1, 4, 4, 3, 1, 1), 1, (4, 0, 1, 0)),              # one pixel, every tap but the centre outside the image, the K-1 clamp
    ((1, 3, 5, 4, 4, 1, 1, 0), 15, (4, 0, 1, 0)),             # one partial tile, odd K
    ((1, 4, 8, 8, 8, 1, 1, 0), 32, (8, 0, 1, 0)),             # exactly one tile
    ((1, 3, 11, 8, 8, 1, 1, 0), 33, (8, 0, 1, 0)),            # the second tile holds one pixel
    ((3, 5, 7, 8, 2, 3, 1, 1), 105, (2, 0, 1, 0)),            # cout = 2 (4-byte stores), K % 32 = 9, a tile straddles samples
    ((1, 16, 16, 4, 4, 1, 1, 0), 256, (4, 0, 2, 0)),          # two slabs: the combine's tail loop only
    ((1, 16, 17, 8, 64, 3, 1, 1), 272, (64, 0, 2, 0)),        # splits of 5 and 4 tiles, the <64> kernel with a full column tile
    ((1, 24, 32, 4, 4, 1, 1, 0), 768, (4, 0, 6, 0)),          # six slabs: one unrolled group of four and a tail of two
    ((2, 20, 26, 4, 8, 3, 1, 1), 1040, (8, 0, 7, 0)),         # seven slabs, the last split 3 tiles
    ((5, 33, 37, 8, 12, 3, 2, 1), 1615, (12, 0, 11, 0)),      # the last split ONE tile; stride 2, odd sizes, K % 32 = 15
    ((10, 12, 16, 32, 132, 3, 1, 1), 1920, (128, 4, 15, 15)),  # batch 10; the 128-wide part and a 4-column tail
    ((1, 40, 41, 16, 388, 1, 1, 0), 1640, (384, 4, 13, 13)),  # 384 + 4 columns
    ((1, 64, 131, 4, 68, 1, 1, 0), 8384, (68, 0, 53, 0)),     # the last split 2 tiles, the <128> kernel with 68 columns
    ((10, 24, 32, 4, 2, 3, 1, 1), 7680, (2, 0, 60, 0)),       # cout = 2 under split-K: slabs and combine of 2-float rows
    ((1, 128, 129, 4, 4, 1, 1, 0), 16512, (4, 0, 129, 0)),
    ((1, 128, 256, 4, 4, 1, 1, 0), 32768, (4, 0, 256, 0)),    # the cap
    ((10, 6, 8, 128, 256, 4, 2, 1), 120, (256, 0, 1, 0)),     # the deconv's geometry, M = 2048: 16 row tiles
    ((1, 20, 24, 64, 64, 7, 2, 3), 120, (64, 0, 1, 0)),       # 7x7, M = 3136: a last row tile of 64 rows
]
# (B, H, W, cin, cout), T = B*ceil(H/2)*ceil(W/2), ksplit of the 16-plane batched launch
WINO_WGRAD_SPLIT_CASES = [
    ((1, 2, 2, 4, 4), 1, 1),                 # one tile
    ((1, 3, 5, 8, 4), 6, 1),                 # ragged tiles
    ((3, 9, 8, 32, 64), 60, 1),
    ((2, 33, 20, 32, 192), 340, 2),          # two column tiles per plane, splits of 6 and 5 K-tiles
    ((1, 64, 66, 4, 8), 1056, 7),            # 16 x 7 slabs, the last split 3 tiles
]


def wgrad_split_features(cases):
    """what a table of (case, K, split) rows reaches in wgrad_mfma.hip, by name"""
    hit = set()
    for case, K, (n_main, n_tail, ks, ks_tail) in cases:
        cout, M = case[4], case[5] * case[5] * case[3]
        ktiles = (K + 31) // 32
        kts = (ktiles + ks - 1) // ks                        # K-tiles per split (the kernel's own two lines)
        last = ktiles - (ks - 1) * kts
        assert 1 <= last <= kts
        hit.add(f"ks={ks}")
        if ks > 4:
            hit.add(f"ks=4n+{ks % 4}")                       # the combine's unrolled groups of four, then a tail of ks % 4
        if ks > 1 and last == 1:
            hit.add("one-tile last split")
        if ks > 1 and 1 < last < kts:
            hit.add("short last split")
        hit.add("one tile per split" if kts == 1 else "several tiles per split")
        hit.add("K=1" if K == 1 else "K<32" if K < 32 else "K=32" if K == 32 else "K=33" if K == 33 else "K>33")
        if K % 32:
            hit.add("partial last tile")
        if K > 33 and K % 2:
            hit.add("odd K")
        if cout % 4:
            hit.add("cout%4 with ks=1" if ks == 1 else "cout%4 with ks>1")
        if n_tail:
            hit.add("main part plus tail")
        hit.add("<64> kernel" if n_main <= 64 else "<128> kernel")
        if M > 128:
            hit.add("several row tiles")
        if M > 128 and M % 128:
            hit.add("partial last row tile")
    return hit


WGRAD_FEATURES = {"ks=1", "ks=2", "ks=4n+0", "ks=4n+1", "ks=4n+2", "ks=4n+3", "ks=256", "one-tile last split", "short last split",
                  "one tile per split", "several tiles per split", "K=1", "K<32", "K=32", "K=33", "partial last tile", "odd K",
                  "cout%4 with ks=1", "cout%4 with ks>1", "main part plus tail", "<64> kernel", "<128> kernel", "several row tiles",
                  "partial last row tile"}


def test_wgrad_split_cases():
    L = _lib.lib()
    for case, K, split in WGRAD_SPLIT_CASES:
        B, Hi, Wi, cin, cout, k, s, p = case
        assert wgrad_case_K(case) == K, case
        assert wgrad_split(k * k * cin, cout, K) == split == wgrad_split(k * k * cin, cout, K, 1), case
        n_main, n_tail, ks, ks_tail = split
        assert n_main + n_tail == cout and (n_tail == 0) == (ks_tail == 0)
        # the workspace the entry point asks for holds the larger of the two launches' slabs
        Ho, Wo = (Hi + 2 * p - k) // s + 1, (Wi + 2 * p - k) // s + 1
        slabs = max(ks * n_main if ks > 1 else 0, ks_tail * n_tail if ks_tail > 1 else 0) * k * k * cin * 4
        assert L.vstab_conv_wgrad_workspace_bytes(B, Ho, Wo, k, cin, cout) >= slabs + 256
    for (B, H, W, cin, cout), T, ks in WINO_WGRAD_SPLIT_CASES:
        assert B * ((H + 1) // 2) * ((W + 1) // 2) == T
        assert wgrad_split(cin, cout, T, 16) == (cout, 0, ks, 0), (B, H, W, cin, cout)
        assert L.vstab_conv3x3_winograd_wgrad_workspace_bytes(B, H, W, cin, cout) >= (16 * ks * cin * cout * 4 if ks > 1 else 0) + 256
    assert {ks for _, _, ks in WINO_WGRAD_SPLIT_CASES} >= {1, 2} and max(ks for _, _, ks in WINO_WGRAD_SPLIT_CASES) > 4


def test_wgrad_split_cases_cover_every_path():
    """a later change of the rule that moves a row off its purpose fails here (or above), not silently in the GPU file"""
    hit = wgrad_split_features(WGRAD_SPLIT_CASES)
    assert hit >= WGRAD_FEATURES, WGRAD_FEATURES - hit


def test_wgrad_split_view_refusals_and_rule():
    L = _lib.lib()
    out = (C.c_int32 * 4)(7, 7, 7, 7)
    assert L.vstab_host_wgrad_split(36, 4, 100, 0, None) == -1
    for bad in ((0, 4, 100, 0), (36, 0, 100, 0), (36, 4, 0, 0), (36, 4, 100, 2), (36, 4, 100, -1), (6, 4, 100, 16), (8, 6, 100, 16)):
        assert L.vstab_host_wgrad_split(*bad, out) == -1 and tuple(out) == (7, 7, 7, 7), bad
    # the column rule: a tail of at most 32 columns behind at least one 128-column tile runs as a launch of its own
    for cout, parts in ((128, (128, 0)), (129, (128, 1)), (160, (128, 32)), (161, (161, 0)), (127, (127, 0)), (388, (384, 4)), (2, (2, 0))):
        assert wgrad_split(64, cout, 4096)[:2] == parts, cout
    # every split the view reports is non-empty: (ks - 1) * ceil(ktiles / ks) < ktiles
    for K in list(range(1, 200)) + [1000, 4095, 4096, 4097, 1 << 20]:
        for M, cout in ((4, 4), (72, 64), (288, 128), (2048, 256), (4608, 512)):
            ks = wgrad_split(M, cout, K)[2]
            ktiles = (K + 31) // 32
            assert 1 <= ks <= 256 and (ks - 1) * ((ktiles + ks - 1) // ks) < ktiles, (M, cout, K, ks)
            assert ks == 1 or ktiles // ks >= 1 and ks <= max(ktiles // 4, 1)


# ---- the training step's forward and input gradient as GEMMs on raw weights (csrc/train_conv_api.cpp: plan_forward, plan_dgrad), as
# vstab_host_train_conv_plan reports them: the launches, the workspace and the gather table the operand is packed through
from tests import train_conv_ref as tcr  # noqa: E402

LAUNCH_FIELDS = "nphase tile vec4 ksplit Mmax N Npad w_off".split()
PHASE_K_FIELDS = PH_FIELDS + "KH NSEG SEG SEGP SEG_STRIDE".split()
TILE_COLS = {0: 128, 1: 64, 2: 32, 3: 128}
SENTINEL = -77


def train_conv_plan_raw(dgrad, B, Hi, Wi, cs_x, cin, k, s, p, out_hw, cs_y, cout, c_off=0, act=0, cap=96, table_cap=None):
    """(return code, the int buffer, the table buffer or None); both buffers start as SENTINEL"""
    buf = (C.c_int32 * 96)(*([SENTINEL] * 96))
    tbl = None if table_cap is None else np.full(table_cap, SENTINEL, np.int32)
    rc = _lib.lib().vstab_host_train_conv_plan(dgrad, B, Hi, Wi, cs_x, cin, k, s, p, out_hw[0], out_hw[1], cs_y, cout, c_off, act, buf, cap,
                                               None if tbl is None else tbl.ctypes.data_as(C.POINTER(C.c_int32)), 0 if tbl is None else len(tbl))
    return rc, list(buf), tbl


def train_conv_plan(*args, **kw):
    """the plan as a dict (launches: list of dicts with their phases) and its gather table (length 0 for a blocked operand)"""
    rc, buf, _ = train_conv_plan_raw(*args, **kw)
    assert rc > 0, (args, kw, _lib.lib().vstab_last_error(None))
    d = dict(zip("launches packed_floats part_floats blocked_K tbl_nfast ws256 table_entries".split(), buf[:7]))
    at, d["launch"] = 7, []
    for _ in range(d["launches"]):
        la = dict(zip(LAUNCH_FIELDS, buf[at:at + 8]))
        la["ph"] = [dict(zip(PHASE_K_FIELDS, buf[at + 8 + 12 * f:at + 20 + 12 * f])) for f in range(la["nphase"])]
        at += 8 + 12 * la["nphase"]
        d["launch"].append(la)
    assert at == rc and all(v == SENTINEL for v in buf[rc:])
    rc2, buf2, tbl = train_conv_plan_raw(*args, **kw, table_cap=d["table_entries"])
    assert rc2 == rc and buf2 == buf
    return d, tbl


def plan_tiles(d):
    """128-row tiles of every phase of every launch, in column tiles of the launch's own width"""
    return sum(-(-ph["M"] // 128) * (la["Npad"] // TILE_COLS[la["tile"]]) for la in d["launch"] for ph in la["ph"])


@pytest.mark.parametrize("i", range(len(tcr.PHASE_CASES)))
def test_odd_k_stride2_dgrad_plan_is_the_one_the_case_names(i):
    """what tests/test_gpu_train_conv_edges.py section B assumes: 'merged' rows run as ONE launch of all parity phases, the others as
    one launch per non-empty parity phase, and the tile count that decides it is the recorded one"""
    B, Hi, Wi, cin, cout, k, p, _, tiles, per_phase = tcr.PHASE_CASES[i]
    hw = tcr.phase_out_hw(tcr.PHASE_CASES[i])
    for sliced in (False, True):            # the plain call, and the accumulating call into a slice (cg_off moves a pointer only)
        d, _ = train_conv_plan(1, B, Hi, Wi, cin + 8 * sliced, cin, k, 2, p, hw, cout + 8 * sliced, cout, c_off=4 * sliced, act=int(sliced))
        nonempty = sum(1 for py in range(2) for px in range(2)
                       if min((Hi - py + 1) // 2, (Wi - px + 1) // 2, (k - ((py + p) & 1) + 1) // 2, (k - ((px + p) & 1) + 1) // 2) >= 1)
        assert d["launches"] == (nonempty if per_phase else 1)
        assert [la["nphase"] for la in d["launch"]] == ([1] * nonempty if per_phase else [nonempty])
        assert plan_tiles(d) == tcr.dgrad_plan_tiles(B, Hi, Wi, cin, k, p) == tiles
        assert (tiles > tcr.PHASE_THRESHOLD) == per_phase
        if not per_phase:                   # split-K sized for the phases together: 512 / tiles, at most a quarter of the shortest reduction
            kt_min = min(ph["KH"] * ph["NSEG"] * ph["SEGP"] // 32 for ph in d["launch"][0]["ph"])
            assert d["launch"][0]["ksplit"] == max(1, min(512 // tiles, max(1, kt_min // 4)))


def _train_conv_geometries():
    """(dgrad, B, Hi, Wi, cs_x, cin, k, s, p, out_hw, cs_y, cout, c_off, act): sections A and B of the GPU test, as it calls them (contiguous
    tensors; slices of wider pixels on both sides with the accumulating epilogue), for the forward and the input gradient"""
    geo = [(c, tcr.extra_out_hw(c, d)) for c in tcr.EXTRA_CASES for d in tcr.EXTRA_DELTAS]
    geo += [((c[0], c[1], c[2], c[3], c[4], c[5], 2, c[6]), tcr.phase_out_hw(c)) for c in tcr.PHASE_CASES]
    out = []
    for (B, Hi, Wi, cin, cout, k, s, p), hw in geo:
        for dgrad in (0, 1):
            out.append((dgrad, B, Hi, Wi, cin, cin, k, s, p, hw, cout, cout, 0, 0))
            out.append((dgrad, B, Hi, Wi, cin + 8, cin, k, s, p, hw, cout + 12, cout, 4, 3 if not dgrad else 1))
    return out


def test_train_conv_plans_tables_and_workspace():
    r256 = lambda n: (n + 255) // 256 * 256
    seen = set()
    for g in _train_conv_geometries():
        dgrad, B, Hi, Wi, cs_x, cin, k, s, p, hw, cs_y, cout, c_off, act = g
        d, tbl = train_conv_plan(*g[:12], c_off=c_off, act=act)
        numel = k * k * cin * cout
        la0 = d["launch"][0]
        assert all(la["N"] == (cin if dgrad else cout) and la["Npad"] == la0["Npad"] for la in d["launch"])
        # the packed operand is the phases' operands one after the other
        sizes = [ph["KH"] * ph["NSEG"] * (ph["SEGP"] // 32) * la["Npad"] * 32 for la in d["launch"] for ph in la["ph"]]
        assert sum(sizes) == d["packed_floats"]
        assert [la["w_off"] for la in d["launch"]] == [sum(sizes[:n]) for n in range(d["launches"])] or d["launches"] == 1
        # workspace: operand, bias vector of Npad floats, split-K slabs, each rounded to 256 bytes, and 256 for the caller's alignment
        assert d["ws256"] * 256 == r256(4 * d["packed_floats"]) + r256(4 * la0["Npad"]) + r256(4 * d["part_floats"]) + 256
        slabs = [la["nphase"] * la["ksplit"] * la["Mmax"] * la["Npad"] if la["ksplit"] > 1 else 0 for la in d["launch"]]
        assert d["part_floats"] == max(slabs)
        if d["blocked_K"] > 0:
            assert not dgrad and d["blocked_K"] == k * k * cin and d["table_entries"] == 0 and len(tbl) == 0 and not d["tbl_nfast"]
            seen.add("blocked")
            continue
        assert d["table_entries"] == d["packed_floats"] == len(tbl)
        assert tbl.min() >= 0 and tbl.max() <= numel
        # every filter element is gathered exactly once: over the parity phases together, each tap belongs to one of them
        assert np.array_equal(np.bincount(tbl, minlength=numel + 1)[1:], np.ones(numel, np.int64)), g
        seen.add(("dgrad" if dgrad else "forward", "table"))
        if dgrad:
            assert not d["tbl_nfast"]
            continue
        # forward: logical reduction index kk of column n is tap (t, kx), channel ci of the USED channels, wherever the K layout puts it
        ph = la0["ph"][0]
        KT, Np = ph["KH"] * ph["NSEG"] * ph["SEGP"] // 32, la0["Npad"]
        t3 = tbl.reshape(KT, Np, 32)
        unsw = np.array([[swz32(n, q) for q in range(32)] for n in range(Np)])
        logical = np.take_along_axis(t3, np.broadcast_to(unsw, t3.shape), axis=2).transpose(0, 2, 1).reshape(KT * 32, Np)
        kk = np.arange(KT * 32)
        t, sg, q = kk // (ph["NSEG"] * ph["SEGP"]), kk // ph["SEGP"] % ph["NSEG"], kk % ph["SEGP"]
        kx, ci = (q // cin, q % cin) if ph["NSEG"] == 1 else (sg, q)
        assert ph["SEG"] == (k * cin if ph["NSEG"] == 1 else cin) and (ph["NSEG"] == 1) == (cs_x == cin)
        want = 1 + (((t * k + kx) * cin + ci) * cout)[:, None] + np.arange(Np)[None, :]
        want = np.where((q < ph["SEG"])[:, None] & (np.arange(Np) < cout)[None, :], want, 0)
        assert np.array_equal(logical, want), g
        seen.add("tap mode" if cs_x > cin else "run mode")
    assert seen >= {"blocked", ("dgrad", "table"), ("forward", "table"), "tap mode", "run mode"}, seen


def test_train_conv_plan_refusals_leave_the_output_untouched():
    E_SHAPE, E_NOMEM = -1, -4
    B, Hi, Wi, cin, cout, k, s, p = tcr.EXTRA_CASES[0]
    hw = tcr.extra_out_hw(tcr.EXTRA_CASES[0], (0, 0))
    ok = (B, Hi, Wi, cin, cin, k, s, p, hw, cout, cout)
    n_tbl = train_conv_plan(1, *ok)[0]["table_entries"]
    bad = [
        ((1, B, Hi, Wi, cin, cin, k, 3, p, (tcr.min_out(Hi, k, 3, p), tcr.min_out(Wi, k, 3, p)), cout, cout), E_SHAPE),   # stride 3 in the input gradient
        ((1, B, Hi, Wi, cin, cin, k, s, p, (hw[0] + 2, hw[1]), cout, cout), E_SHAPE),                 # two extra rows
        ((0, B, Hi, Wi, cin, cin, k, s, p, (hw[0] + 2, hw[1]), cout, cout), E_SHAPE),
        ((0, B, Hi, Wi, cin, cin, k, s, p, (hw[0], hw[1] + 2), cout, cout), E_SHAPE),
        ((1, 1, 9, 11, 8, 8, 3, 1, 1, (10, 11), 8, 8), E_SHAPE),                                     # stride 1 takes no extra row in the input gradient
        ((1, 1, 4096, 4096, 32, 32, 3, 2, 1, (2048, 2048), 32, 32), E_SHAPE),                         # dx at exactly 2 GiB
        ((0, 1, 4096, 4096, 32, 32, 3, 2, 1, (2048, 2048), 32, 32), E_SHAPE),                         # x at exactly 2 GiB
        ((0, 1, 2048, 2048, 32, 32, 3, 1, 1, (2048, 2049), 128, 32), E_SHAPE),                        # y reaches 2 GiB through its extra column only
    ]
    for args, code in bad:
        rc, buf, tbl = train_conv_plan_raw(*args, table_cap=64)
        assert rc == code and all(v == SENTINEL for v in buf) and (tbl == SENTINEL).all(), args
    assert 4096 * 4096 * 32 * 4 == 1 << 31 and 2048 * 2048 * 128 * 4 == 1 << 31
    assert train_conv_plan_raw(1, 1, 4096, 4095, 32, 32, 3, 2, 1, (2048, 2048), 32, 32)[0] > 0        # one column less fits
    for kw in (dict(cap=7 + 8 + 4 * 12 - 1), dict(table_cap=n_tbl - 1)):
        rc, buf, tbl = train_conv_plan_raw(1, *ok, **kw)
        assert rc == E_NOMEM and all(v == SENTINEL for v in buf) and (tbl is None or (tbl == SENTINEL).all())
    assert _lib.lib().vstab_host_train_conv_plan(1, *ok[:8], hw[0], hw[1], cout, cout, 0, 0, None, 96, None, 0) == -6       # VSTAB_E_STATE, as every NULL buffer
