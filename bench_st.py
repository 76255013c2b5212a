#!/usr/bin/env python3
"""The spatial_transformer.py samplers at configs[2]'s size (B = 32, 720 x 1280 x 3): per variant the median time of one call
over HIP events (>= 20 timed calls after warm-up), algorithmic bytes (12 read + 12 written per output pixel) and the fraction
of 8 TB/s.  Prints one JSON line.  AffineTransformer with the bilinear sampler is the existing kernel, the yardstick."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated variant names (default: all)")
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
    print(json.dumps({"bench": "spatial_transformer_samplers", "batch": B, "height": H, "width": W, "channels": 3,
                      "iters": args.iters, "device": torch.cuda.get_device_name(0), "variants": rows}))


if __name__ == "__main__":
    main()
