#!/usr/bin/env python3
"""training.warp_flow_backward for 3-channel frames at the benchmark's output resolution (B = 8, 512 x 512) and at B = 16, 1080 x 1920:
per case and flow the median time over HIP events (>= 20 timed calls after warm-up, the calls taking turns) of the forward
warp_flow.tf_warp and of the backward in its three forms -- d flow only (the tile kernel; also timed on the one-thread-per-pixel
kernel through VSTAB_WARP_BWD_NO_TILE, the library's A/B switch), d img only, both -- the backward / forward ratio, and the
algorithmic bytes as a fraction of 8 TB/s: forward 32 B per pixel; d flow 40 (12 dout + 8 flow + 12 of gathers + 8 written); d img
20 read + 12 zeroed + four 12-byte atomic read-modify-writes (48 modified; counted as 80); both 40 + 60.  Flows: "smooth" (sinusoids
of a few pixels) and "random" (independent N(0, 3) per pixel).  Prints one JSON line.  Not part of bench.py's workload."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ssim import PEAK_GBS, time_interleaved   # noqa: E402
from coupe.optical_flow_based_deep_video_stabilization_amd import training, warp_flow   # noqa: E402

CASES = ((8, 512, 512), (16, 1080, 1920))
SWITCH = "VSTAB_WARP_BWD_NO_TILE"
BYTES = {"forward": 32.0, "d_flow": 40.0, "d_img": 80.0, "both": 100.0}


def flows(B, H, W, g):
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    smooth = torch.stack([3.0 * torch.sin(yy / 50.0) * torch.cos(xx / 70.0), 2.0 * torch.cos(yy / 40.0 + xx / 90.0)], -1)
    return {"smooth": smooth.expand(B, H, W, 2).contiguous().cuda(), "random": (3.0 * torch.randn(B, H, W, 2, generator=g)).cuda()}


def pixel_form(fn):
    def run():
        os.environ[SWITCH] = "1"
        try:
            return fn()
        finally:
            del os.environ[SWITCH]
    return run


def case_rows(B, H, W, iters, warmup):
    g = torch.Generator().manual_seed(B + H)
    img, dout = torch.rand(B, H, W, 3, generator=g).cuda(), torch.randn(B, H, W, 3, generator=g).cuda()
    d_img = torch.empty_like(img)          # written in place every call: the zeroing is timed, an allocation is not
    out = {"batch": B, "height": H, "width": W, "flows": {}}
    for name, flow in flows(B, H, W, g).items():
        def d_img_only():
            d_img.zero_()
            return training.warp_flow_backward(img, flow, dout, need_flow=False, d_img=d_img)

        def both():
            d_img.zero_()
            return training.warp_flow_backward(img, flow, dout, d_img=d_img)

        fns = {"forward": lambda: warp_flow.tf_warp(img, flow, H, W),
               "d_flow": lambda: training.warp_flow_backward(img, flow, dout, need_img=False), "d_img": d_img_only, "both": both}
        fns["d_flow_pixel"] = pixel_form(fns["d_flow"])
        us = time_interleaved(fns, iters, warmup)
        npix = B * H * W
        rows = {k: {"us": round(v, 1), "x_forward": round(v / us["forward"], 3),
                    "frac_8TBs": round(BYTES[k.replace("_pixel", "")] * npix / (v * 1e-6) / 1e9 / PEAK_GBS, 4)} for k, v in us.items()}
        out["flows"][name] = rows
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp_grad.py needs a GPU")
    result = {"bench": "warp_flow_backward_c3", "iters": args.iters, "device": torch.cuda.get_device_name(0),
              "cases": [case_rows(B, H, W, args.iters, args.warmup) for B, H, W in CASES]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
