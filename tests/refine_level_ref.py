"""Plain float64 references of a refinement level's two hand-written pieces (csrc/winograd_ops.hip, csrc/flow_ops.hip), torch / numpy on the
CPU, pinned by tests/test_refine_level_ref_cpu.py and used by tests/test_gpu_refine_level.py:

  deconv_ref       the 4x4 stride-2 SAME transposed convolution (model.py:850-851 ...) + bias + leaky relu, into a channel slice
  wdec_emulated    the same through the Winograd F(2x2,2x2) algebra winograd_ops.hip documents, statement for statement, with the tile
                   grid and the per-position clipping rule of wdec_geom -- so the rule can be proved without a GPU
  predict_up_ref   predict_flowN + upsample_flowN from the tap table's split-K slabs (flow_ops.hip's predict_up_body), with the number of
                   addends and the sum of their magnitudes per flow element (the GPU test's tolerance)
  upsample_ref     its last stage alone: the 2 -> 2 transposed convolution of a given flow, with the sum of magnitudes per element

NHWC tensors; filters in the reference's layouts: W [4][4][cout][cin] (DeConv2dLayer), taps T[.., 2 (3 dy + dx) + o]."""
import numpy as np
import torch
import torch.nn.functional as F


def deconv_ref(x, W, bias, act, out_hw, out=None, c_off=0):
    """x [B,Hi,Wi,cs >= cin] (the first cin channels count), W [4,4,cout,cin], bias [cout] or None, act 0 / 1 (leaky relu 0.1) ->
    y [B,Ho,Wo,cout] float64: y[oy,ox,co] = b + sum x[iy,ix,ci] W[ky,kx,co,ci] over oy = 2 iy + ky - 1, cropped to out_hw.  With `out`
    ([B,Ho,Wo,cs_out] float64) the result is also written into its channels c_off .. c_off + cout."""
    W = torch.as_tensor(W).double()
    cout, cin = W.shape[2], W.shape[3]
    xn = torch.as_tensor(x).double()[..., :cin].permute(0, 3, 1, 2)
    y = F.conv_transpose2d(xn, W.permute(3, 2, 0, 1), None if bias is None else torch.as_tensor(bias).double(), stride=2, padding=1)
    Ho, Wo = out_hw
    assert Ho in (2 * xn.shape[2] - 1, 2 * xn.shape[2]) and Wo in (2 * xn.shape[3] - 1, 2 * xn.shape[3])
    y = y[:, :, :Ho, :Wo].permute(0, 2, 3, 1).contiguous()
    if act:
        y = torch.maximum(y, 0.1 * y)
    if out is not None:
        out[..., c_off:c_off + cout] = y
    return y


def wdec_geom(Hi, Wi, Ho, Wo):
    """the tile grid and, per position row / column, the number of tiles that are not identically zero (vstab_internal.h: wdec_geom)"""
    NTy, NTx = Ho // 4 + 1, Wo // 4 + 1
    nty = [min(NTy, Hi // 2 + 1)] + [min(NTy, (Hi + 1) // 2)] * 2
    ntx = [min(NTx, Wi // 2 + 1)] + [min(NTx, (Wi + 1) // 2)] * 2
    return dict(NTy=NTy, NTx=NTx, nty=nty, ntx=ntx)


def wdec_emulated(x, W, out_hw, geom=None):
    """The transposed convolution through Winograd F(2x2,2x2), in float64 numpy.  Per axis: tiles NT = Ho/4 + 1; tile t reads
    d = (x[2t-1], x[2t], x[2t+1]) (zeros outside), v = (d0 - d1, d1, d1 - d2); output parity p has the taps g = (W[3-p], W[1-p]),
    u = (g0, g0 + g1, g1); m_i = v_i u_i, dropped (read as zero) for t >= nt[i]; the pair (m0 + m1, m1 - m2) lands at 4t + 2a - p,
    a = 0, 1.  In 2-D the transforms nest and m_ij = sum_ci v_ij u_ij.  Returns y [B,Ho,Wo,cout] with NaN where nothing was written."""
    x = np.asarray(x, np.float64)
    W = np.asarray(W, np.float64)
    B, Hi, Wi, _ = x.shape
    cout, cin = W.shape[2], W.shape[3]
    Ho, Wo = out_hw
    g = geom or wdec_geom(Hi, Wi, Ho, Wo)
    NTy, NTx = g["NTy"], g["NTx"]
    xp = np.zeros((B, 2 * NTy + 2, 2 * NTx + 2, cin))                     # xp[r] = x[r - 1]
    xp[:, 1:1 + Hi, 1:1 + Wi] = x[..., :cin]
    d = [[xp[:, i:i + 2 * NTy:2, j:j + 2 * NTx:2] for j in range(3)] for i in range(3)]          # d[i][j][b, ty, tx, ci]
    r = [[d[0][j] - d[1][j] for j in range(3)], [d[1][j] for j in range(3)], [d[1][j] - d[2][j] for j in range(3)]]
    v = [[r[i][0] - r[i][1], r[i][1], r[i][1] - r[i][2]] for i in range(3)]
    y = np.full((B, Ho, Wo, cout), np.nan)
    for py in range(2):
        for px in range(2):
            gg = [[W[3 - py - 2 * a, 3 - px - 2 * b] for b in range(2)] for a in range(2)]      # gg[a][b][co, ci]
            ur = [[gg[0][b] for b in range(2)], [gg[0][b] + gg[1][b] for b in range(2)], [gg[1][b] for b in range(2)]]
            u = [[ur[i][0], ur[i][0] + ur[i][1], ur[i][1]] for i in range(3)]
            m = [[None] * 3 for _ in range(3)]
            for i in range(3):
                for j in range(3):
                    mij = np.einsum("byxc,oc->byxo", v[i][j], u[i][j])
                    mij[:, g["nty"][i]:] = 0.0                                # the tiles this position row / column does not compute
                    mij[:, :, g["ntx"][j]:] = 0.0
                    m[i][j] = mij
            s = [[m[0][j] + m[1][j] for j in range(3)], [m[1][j] - m[2][j] for j in range(3)]]
            for a in range(2):
                for b in range(2):
                    blk = s[a][0] + s[a][1] if b == 0 else s[a][1] - s[a][2]
                    oy = 4 * np.arange(NTy) + 2 * a - py
                    ox = 4 * np.arange(NTx) + 2 * b - px
                    oky, okx = (oy >= 0) & (oy < Ho), (ox >= 0) & (ox < Wo)
                    y[:, oy[oky][:, None], ox[okx][None, :]] = blk[:, oky][:, :, okx]
    return y


def legacy_axis(n_in, n_out):
    """TF-1.10 ResizeBilinear (align_corners=False), one axis, coordinates in fp32 exactly as legacy_coord (csrc/resample_coords.h):
    f = float(o) * (float(n_in) / float(n_out)), lo = min(floor(f), n_in - 1), hi = min(lo + 1, n_in - 1), t = f - floor(f)"""
    scale = np.float32(n_in) / np.float32(n_out)
    f = (np.arange(n_out, dtype=np.float32) * scale).astype(np.float32)
    fl = np.floor(f)
    lo = np.minimum(fl.astype(np.int64), n_in - 1)
    hi = np.minimum(lo + 1, n_in - 1)
    return lo, hi, (f - fl).astype(np.float32).astype(np.float64)


def legacy_sample(prev, h, w):
    """prev [B,ph,pw,2] -> (u, mag) [B,h,w,2] float64: the legacy-bilinear sample top + (bot - top) ty, top = tl + (tr - tl) tx, and the
    same expression on magnitudes with every difference replaced by a sum (what bounds each intermediate of the fp32 evaluation)"""
    p = torch.as_tensor(prev).double()
    ylo, yhi, ty = legacy_axis(p.shape[1], h)
    xlo, xhi, tx = legacy_axis(p.shape[2], w)
    ty = torch.from_numpy(ty).view(1, h, 1, 1)
    tx = torch.from_numpy(tx).view(1, 1, w, 1)
    tl, tr, bl, br = p[:, ylo][:, :, xlo], p[:, ylo][:, :, xhi], p[:, yhi][:, :, xlo], p[:, yhi][:, :, xhi]
    top, bot = tl + (tr - tl) * tx, bl + (br - bl) * tx
    atop, abot = tl.abs() + (tr.abs() + tl.abs()) * tx, bl.abs() + (br.abs() + bl.abs()) * tx
    return top + (bot - top) * ty, atop + (abot + atop) * ty


def upsample_ref(flow, up_w, up_b, out_hw):
    """flow [B,h,w,2], up_w [4,4,co,ci], up_b [2] -> (up, mag) [B,oh,ow,2] float64: the 4x4 stride-2 SAME transposed convolution + bias
    cropped to out_hw, and |b| + sum |f w| over the same taps"""
    f = torch.as_tensor(flow).double().permute(0, 3, 1, 2)
    w = torch.as_tensor(up_w).double().reshape(4, 4, 2, 2).permute(3, 2, 0, 1)
    b = torch.as_tensor(up_b).double()
    oh, ow = out_hw
    up = F.conv_transpose2d(f, w, b, stride=2, padding=1)[:, :, :oh, :ow].permute(0, 2, 3, 1).contiguous()
    mag = F.conv_transpose2d(f.abs(), w.abs(), b.abs(), stride=2, padding=1)[:, :, :oh, :ow].permute(0, 2, 3, 1).contiguous()
    return up, mag


def predict_up_ref(slabs, bias2, prev, up_w, up_b, out_hw):
    """slabs [ks,B,h,w,>=18] (the split-K slabs of the tap table; only columns 0..17 are read), bias2 [2], prev [B,ph,pw,2] or None ->
    dict(flow [B,h,w,2], up [B,oh,ow,2], n [B,h,w,2] int, S [B,h,w,2]):
      flow[y,x,o] = b[o] + sum over the in-image taps (dy, dx) and the slabs of T[y+dy-1, x+dx-1, 2 (3 dy + dx) + o]  [+ 2 u]
      u = the legacy-bilinear sample of prev (coordinates in fp32, values in float64), up = upsample_ref(flow)
      n = the number of addends of flow (1 + ks * taps in the image + 2 with prev), S = the sum of their magnitudes (legacy_sample's
      magnitude form for u)."""
    T = torch.as_tensor(slabs).double()[..., :18]
    ks, B, h, w, _ = T.shape
    Ts, Ta = T.sum(0), T.abs().sum(0)
    b = torch.as_tensor(bias2).double()
    flow = b.view(1, 1, 1, 2).expand(B, h, w, 2).clone()
    S = b.abs().view(1, 1, 1, 2).expand(B, h, w, 2).clone()
    n = torch.ones(B, h, w, 2, dtype=torch.int64)
    for dy in range(3):
        for dx in range(3):
            y0, y1 = max(0, 1 - dy), min(h, h + 1 - dy)               # outputs whose tap (dy, dx) lies in the image
            x0, x1 = max(0, 1 - dx), min(w, w + 1 - dx)
            if y0 >= y1 or x0 >= x1:
                continue
            c = 2 * (3 * dy + dx)
            flow[:, y0:y1, x0:x1] += Ts[:, y0 + dy - 1:y1 + dy - 1, x0 + dx - 1:x1 + dx - 1, c:c + 2]
            S[:, y0:y1, x0:x1] += Ta[:, y0 + dy - 1:y1 + dy - 1, x0 + dx - 1:x1 + dx - 1, c:c + 2]
            n[:, y0:y1, x0:x1] += ks
    if prev is not None:
        u, mag = legacy_sample(prev, h, w)
        flow = flow + 2.0 * u
        S = S + 2.0 * mag
        n = n + 2
    up, _ = upsample_ref(flow, up_w, up_b, out_hw)
    return dict(flow=flow, up=up, n=n, S=S)
