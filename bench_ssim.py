#!/usr/bin/env python3
"""utils.tf_ssim in its mean form (size 9, sigma 0.5) at B = 8, 512 x 512 and B = 16, 1080 x 1920: per case the median time over HIP
events (>= 20 timed calls after warm-up) of the forward alone and of forward + backward (both image gradients), the bytes that have
to move algorithmically -- forward: the two images read, nothing written (8 B per pixel); forward + backward: the images read again
and both gradients written (24 B per pixel) -- and that as a fraction of 8 TB/s.  For scale the same value computed by composing
torch ops on the GPU (five conv2d calls with the 2-D window plus pointwise ops, and autograd for its backward) is timed interleaved
with the library's calls; it is a comparison, not a gate.  Prints one JSON line.  Not part of bench.py's workload."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coupe.optical_flow_based_deep_video_stabilization_amd import utils   # noqa: E402

PEAK_GBS = 8000.0
CASES = ((8, 512, 512), (16, 1080, 1920))


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


def torch_ssim_mean(x, y, win):
    """the same value from torch ops: x, y [B,1,H,W], win [1,1,k,k]"""
    mu1, mu2 = F.conv2d(x, win), F.conv2d(y, win)
    s1 = F.conv2d(x * x, win) - mu1 * mu1
    s2 = F.conv2d(y * y, win) - mu2 * mu2
    s12 = F.conv2d(x * y, win) - mu1 * mu2
    c3 = 0.03 ** 2 / 2
    return ((s12 * s12 + c3) / (s1 * s2 + c3)).mean()


def case_rows(B, H, W, iters, warmup):
    g = torch.Generator().manual_seed(B + H)
    x = torch.rand(B, H, W, 1, generator=g).cuda()
    y = (x.cpu() * 0.8 + 0.2 * torch.rand(B, H, W, 1, generator=g)).cuda()
    xg, yg = x.clone().requires_grad_(True), y.clone().requires_grad_(True)
    win = utils._tf_fspecial_gauss(9, 0.5).reshape(1, 1, 9, 9).cuda()
    xt, yt = x.reshape(B, 1, H, W), y.reshape(B, 1, H, W)                # one channel: NHWC and NCHW are the same bytes
    xtg, ytg = xt.clone().requires_grad_(True), yt.clone().requires_grad_(True)

    def fwd_bwd():
        return torch.autograd.grad(utils.tf_ssim(xg, yg), (xg, yg))

    def torch_fwd():
        with torch.no_grad():
            return torch_ssim_mean(xt, yt, win)

    def torch_fwd_bwd():
        return torch.autograd.grad(torch_ssim_mean(xtg, ytg, win), (xtg, ytg))

    value, tvalue = float(utils.tf_ssim(x, y)), float(torch_fwd())
    us = time_interleaved({"forward": lambda: utils.tf_ssim(x, y), "torch_forward": torch_fwd, "forward_backward": fwd_bwd,
                           "torch_forward_backward": torch_fwd_bwd}, iters, warmup)
    npix = B * H * W
    nbytes = {"forward": 8.0, "torch_forward": 8.0, "forward_backward": 24.0, "torch_forward_backward": 24.0}
    rows = {k: {"us": round(v, 1), "alg_bytes": int(nbytes[k] * npix), "frac_8TBs": round(nbytes[k] * npix / (v * 1e-6) / 1e9 / PEAK_GBS, 4)}
            for k, v in us.items()}
    rows["forward"]["x_torch"] = round(us["forward"] / us["torch_forward"], 3)
    rows["forward_backward"]["x_torch"] = round(us["forward_backward"] / us["torch_forward_backward"], 3)
    return {"batch": B, "height": H, "width": W, "value": value, "torch_value": tvalue, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ssim.py needs a GPU")
    result = {"bench": "tf_ssim_mean_form", "size": 9, "sigma": 0.5, "iters": args.iters, "device": torch.cuda.get_device_name(0),
              "cases": [case_rows(B, H, W, args.iters, args.warmup) for B, H, W in CASES]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
