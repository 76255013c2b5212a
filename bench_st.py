#!/usr/bin/env python3
"""The spatial_transformer.py samplers at configs[2]'s size (B = 32, 720 x 1280 x 3): per variant the median time of one call
over HIP events (>= 20 timed calls after warm-up), algorithmic bytes (12 read + 12 written per output pixel) and the fraction
of 8 TB/s.  Prints one JSON line.  AffineTransformer with the bilinear sampler is the existing kernel, the yardstick.
--backward adds the gradients of the affine bilinear transformer at the same shape (rows "backward"): d img (four global atomics
per pixel-channel), d theta, both together, and torch's own grid_sample backward (NCHW, bilinear, zeros, align_corners=True) for scale -- an independent implementation of a comparable op,
not a gate; and the gradients of ElasticTransformer (g = 4, bilinear) at the same shape (rows "elastic_g4_*": time and algorithmic
bytes only -- the thin-plate spline is bound by logf, not by HBM, so a fraction of 8 TB/s would say nothing); and those of warp.py's
homography warp under a near-identity homography (rows "homography_*": d img, d M, both).
--volume adds the 3-D volume transformer (rows "volume"): AffineVolumeTransformer at B = 4, 256^3, C = 1 under an oblique rotation of
about 10 degrees plus a small shift -- forward by theta, d vol, d theta, both gradients -- with torch's 5-D grid_sample (bilinear,
zeros, align_corners=True) forward timed interleaved for scale.  The forward counts 8 algorithmic bytes per output voxel."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coupe.optical_flow_based_deep_video_stabilization_amd import spatial_transformer as st   # noqa: E402

PEAK_GBS = 8000.0


def time_call(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


def time_interleaved(fns, iters, warmup):
    """median us of each call, the calls taking turns (A B A B ...) so that clock and cache state are shared"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for k in fns}
    for i in range(iters):
        for k, fn in fns.items():
            a, b = ev[k][i]
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return {k: statistics.median(a.elapsed_time(b) for a, b in v) * 1e3 for k, v in ev.items()}


def backward_rows(img, th6, out_size, iters, warmup):
    """d img reads dout (12 B / pixel) and adds into an image it first zero-fills (12 B written by the fill + 12 B added per source
    pixel): 36 B per pixel at equal sizes; d theta reads dout and the image: 24 B; both: 48 B."""
    from coupe.optical_flow_based_deep_video_stabilization_amd import training
    import torch.nn.functional as F
    B, H, W, _ = img.shape
    npix = B * out_size[0] * out_size[1]
    dout = torch.rand(B, out_size[0], out_size[1], 3, generator=torch.Generator().manual_seed(2)).cuda()

    def run(need_img, need_theta):
        return lambda: training.st_transform_backward(img, th6, dout, out_size, need_img=need_img, need_theta=need_theta)

    fns = {"d_img": run(True, False), "d_theta": run(False, True), "both": run(True, True)}
    # yardstick: grid_sample's backward for both inputs
    x = img.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    grid = F.affine_grid(th6.reshape(B, 2, 3), (B, 3, out_size[0], out_size[1]), align_corners=True).requires_grad_(True)
    gout = dout.permute(0, 3, 1, 2).contiguous()
    y = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    fns["torch_grid_sample_backward"] = lambda: torch.autograd.grad(y, (x, grid), gout, retain_graph=True)
    us = time_interleaved(fns, iters, warmup)
    nbytes = {"d_img": 36.0, "d_theta": 24.0, "both": 48.0,
              "torch_grid_sample_backward": 48.0 + 16.0}                      # + the grid read and its gradient written
    rows = {k: {"us": round(v, 1), "alg_bytes": int(nbytes[k] * npix), "frac_8TBs": round(nbytes[k] * npix / (v * 1e-6) / 1e9 / PEAK_GBS, 3)}
            for k, v in us.items()}
    # ElasticTransformer, g = 4: the same bytes per pixel as the affine rows (theta, linv_t and the partial rows are noise)
    tps = st.ElasticTransformer(out_size, 4)
    th_tps = ((torch.rand(B, tps.param_dim, generator=torch.Generator().manual_seed(4)) - 0.5) * 0.1).cuda()

    def run_tps(need_img, need_theta):
        return lambda: training.st_elastic_transform_backward(img, th_tps, dout, out_size, 4, tps.L_inv, need_img=need_img, need_theta=need_theta)

    us = time_interleaved({"d_img": run_tps(True, False), "d_theta": run_tps(False, True), "both": run_tps(True, True)}, iters, warmup)
    rows.update({f"elastic_g4_{k}": {"us": round(v, 1), "alg_bytes": int(nbytes[k] * npix)} for k, v in us.items()})

    # the affine transformer's bicubic sampler: the same algorithmic bytes (16 taps per pixel instead of 4 come from the caches)
    def run_bc(need_img, need_theta):
        return lambda: training.st_transform_backward(img, th6, dout, out_size, need_img=need_img, need_theta=need_theta, interp='bicubic')

    us = time_interleaved({"d_img": run_bc(True, False), "d_theta": run_bc(False, True), "both": run_bc(True, True)}, iters, warmup)
    rows.update({f"bicubic_{k}": {"us": round(v, 1), "alg_bytes": int(nbytes[k] * npix)} for k, v in us.items()})
    # warp.py's homography warp (plain form): M = the canonical-to-pixel map of the frame times a near-identity homography; the
    # same bytes per pixel as the affine rows
    ref = torch.tensor([[(W - 1) / 2, 0.0, (W - 1) / 2], [0.0, (H - 1) / 2, (H - 1) / 2], [0.0, 0.0, 1.0]])
    pM = torch.eye(3).repeat(B, 1, 1) + (torch.rand(B, 3, 3, generator=torch.Generator().manual_seed(6)) - 0.5) * 0.02
    M = torch.matmul(ref, pM).cuda()

    def run_h(need_img, need_M):
        return lambda: training.homography_warp_backward(img, M, dout, out_size, need_img=need_img, need_M=need_M)

    us = time_interleaved({"d_img": run_h(True, False), "d_M": run_h(False, True), "both": run_h(True, True)}, iters, warmup)
    hb = {"d_img": 36.0, "d_M": 24.0, "both": 48.0}
    rows.update({f"homography_{k}": {"us": round(v, 1), "alg_bytes": int(hb[k] * npix),
                                     "frac_8TBs": round(hb[k] * npix / (v * 1e-6) / 1e9 / PEAK_GBS, 3)} for k, v in us.items()})
    return rows


def volume_rows(iters, warmup, B=4, n=256):
    """forward: 4 B gathered + 4 B written per output voxel = 8; d vol: dout read, the zero fill and the add = 12; d theta: dout and
    the volume read = 8; both: 16.  The fraction of 8 TB/s is algorithmic bytes over the HIP-event median."""
    import math
    from coupe.optical_flow_based_deep_video_stabilization_amd import training
    import torch.nn.functional as F
    g = torch.Generator().manual_seed(3)
    vol = torch.rand(B, n, n, n, 1, generator=g).cuda()
    dout = torch.rand(B, n, n, n, 1, generator=g).cuda()
    # about 10 degrees about the oblique axis (1, 2, 3) / sqrt(14) (Rodrigues), plus a small shift
    a, k = math.radians(10.0), torch.tensor([1.0, 2.0, 3.0]) / math.sqrt(14.0)
    K = torch.tensor([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = torch.eye(3) + math.sin(a) * K + (1 - math.cos(a)) * (K @ K)
    theta = torch.cat([R, torch.tensor([[0.02], [-0.015], [0.01]])], 1).reshape(1, 12).repeat(B, 1).cuda()
    out_size = (n, n, n)
    tr = st.AffineVolumeTransformer(out_size)

    def bwd(need_vol, need_theta):
        return lambda: training.st3d_transform_backward(vol, theta, dout, out_size, need_vol=need_vol, need_theta=need_theta)

    x = vol.permute(0, 4, 1, 2, 3).contiguous()
    grid = F.affine_grid(theta.reshape(B, 3, 4), (B, 1, n, n, n), align_corners=True)
    fns = {"forward_theta": lambda: tr.transform(vol, theta), "d_vol": bwd(True, False), "d_theta": bwd(False, True), "both": bwd(True, True),
           "torch_grid_sample_forward": lambda: F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=True)}
    us = time_interleaved(fns, iters, warmup)
    nvox = B * n * n * n
    nbytes = {"forward_theta": 8.0, "d_vol": 12.0, "d_theta": 8.0, "both": 16.0, "torch_grid_sample_forward": 8.0 + 12.0}     # + the grid read
    rows = {k: {"us": round(v, 1), "alg_bytes": int(nbytes[k] * nvox), "frac_8TBs": round(nbytes[k] * nvox / (v * 1e-6) / 1e9 / PEAK_GBS, 3)}
            for k, v in us.items()}
    return {"batch": B, "depth": n, "height": n, "width": n, "channels": 1, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variant names (default: all)")
    ap.add_argument("--backward", action="store_true", help="add the gradients of the affine (bilinear and bicubic) and the elastic (g = 4) transformers (rows 'backward')")
    ap.add_argument("--volume", action="store_true", help="add the 3-D volume transformer at B = 4, 256^3, C = 1 (rows 'volume')")
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    B, H, W = args.batch, args.height, args.width
    g = torch.Generator().manual_seed(1)
    img = torch.rand(B, H, W, 3, generator=g).cuda()
    small = lambda n: ((torch.rand(B, n, generator=g) - 0.5) * 0.1).cuda()       # noqa: E731
    th6 = (torch.tensor([1., 0, 0, 0, 1, 0]).repeat(B, 1) + (torch.rand(B, 6, generator=g) - 0.5) * 0.06).cuda()
    out_size = (H, W)
    variants = []
    for m in ("bilinear", "bicubic"):
        variants.append((f"affine_{m}", st.AffineTransformer(out_size, interp_method=m), th6))
    for m in ("bilinear", "bicubic"):
        variants.append((f"affine_symmetry_{m}", st.AffineSymmetryTransformer(out_size, interp_method=m), small(6)))
        variants.append((f"projective_symmetry_{m}", st.ProjectiveSymmetryTransformer(out_size, interp_method=m), small(8)))
        variants.append((f"similarity_{m}", st.SimilarityTransformer(out_size, interp_method=m), small(4)))
    for m in ("bilinear", "bicubic"):
        variants.append((f"elastic_g4_{m}", st.ElasticTransformer(out_size, 4, interp_method=m), small(32)))
    only = set(filter(None, args.only.split(",")))
    rows = {}
    for name, tr, th in variants:
        if only and name not in only:
            continue
        out = tr.transform(img, th)
        npix = out.numel() // 3
        us = time_call(lambda: tr.transform(img, th), args.iters, args.warmup)
        nbytes = 24.0 * npix
        rows[name] = {"us": round(us, 1), "alg_bytes": int(nbytes), "out_shape": list(out.shape),
                      "frac_8TBs": round(nbytes / (us * 1e-6) / 1e9 / PEAK_GBS, 3)}
        del out
    base = rows.get("affine_bilinear", {}).get("us")
    if base:
        for r in rows.values():
            r["x_affine_bilinear"] = round(r["us"] / base, 3)
    result = {"bench": "spatial_transformer_samplers", "batch": B, "height": H, "width": W, "channels": 3,
              "iters": args.iters, "device": torch.cuda.get_device_name(0), "variants": rows}
    if args.backward:
        result["backward"] = backward_rows(img, th6, out_size, args.iters, args.warmup)
    if args.volume:
        result["volume"] = volume_rows(args.iters, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
