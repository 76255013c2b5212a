#!/usr/bin/env python3
"""flow_vis.flow_to_image (img + anglemap, each sample normalised by its own largest radius) at B = 16, 1080 x 1920 and B = 8,
382 x 510: per case the median time over HIP events (>= 20 timed calls after warm-up) of the fused path, of the same call without
the anglemap, and of the call with the radii given (no maximum pass), next to a composition of torch device ops that does the same
arithmetic in the same order and precisions -- what a user would write today -- timed interleaved with the library's calls; it is a
comparison, not a gate.  Algorithmic bytes per pixel: the maximum pass reads the flow (8 B), the colour pass reads it again (8 B)
and writes img (3 B) and anglemap (3 B): 22 B with both outputs, 19 B without the anglemap, 14 B with given radii; each as a
fraction of 8 TB/s.  The share of bytes on which the two paths agree is reported too (they share everything but the atan2
implementation).  Prints one JSON line.  Not part of bench.py's workload."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coupe.optical_flow_based_deep_video_stabilization_amd import flow_vis   # noqa: E402

PEAK_GBS = 8000.0
CASES = ((16, 1080, 1920), (8, 382, 510))


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


def torch_flow_to_image(flow, wheel):
    """the same arithmetic from torch ops: flow [B,H,W,2] float32, wheel [55,3] float64 already divided by 255"""
    B = flow.shape[0]
    u, v = flow[..., 0], flow[..., 1]
    dead = (u.abs() > 1e7) | (v.abs() > 1e7) | torch.isnan(u) | torch.isnan(v)
    u, v = u.masked_fill(dead, 0.0), v.masked_fill(dead, 0.0)
    maxrad = (u * u + v * v).reshape(B, -1).amax(dim=1).sqrt()
    d = torch.where(maxrad > 0, maxrad, torch.full_like(maxrad, 2.0 ** -52)).reshape(B, 1, 1)
    un, vn = u / d, v / d
    rad = (un * un + vn * vn).sqrt()
    a = torch.atan2(-vn, -un) / math.pi
    fk = (a + 1) / 2 * 54 + 1
    k0f = fk.floor()
    k0 = k0f.long().clamp_(1, 55)
    k1 = torch.where(k0 == 55, torch.ones_like(k0), k0 + 1)
    f = (fk - k0f).double().unsqueeze(-1)
    col = (1 - f) * wheel[k0 - 1] + f * wheel[k1 - 1]
    inside = (rad <= 1).unsqueeze(-1)
    col = torch.where(inside, 1 - rad.double().unsqueeze(-1) * (1 - col), 0.75 * col)
    img = (255 * col).floor().masked_fill(dead.unsqueeze(-1), 0.0).to(torch.uint8)
    ang = (a * 127 + 128).to(torch.uint8).unsqueeze(-1).expand(-1, -1, -1, 3).contiguous()
    return img, ang


def case_rows(B, H, W, iters, warmup):
    g = torch.Generator().manual_seed(B + H)
    flow = (torch.randn(B, H, W, 2, generator=g) * 6.0).cuda()
    wheel = (torch.from_numpy(flow_vis.make_color_wheel()) / 255.0).cuda()
    img, ang, radii = flow_vis.flow_to_image(flow, return_maxrad=True)
    timg, tang = torch_flow_to_image(flow, wheel)
    agree = {"img": float((img == timg).double().mean()), "anglemap": float((ang == tang).double().mean())}
    del timg, tang
    us = time_interleaved({"fused": lambda: flow_vis.flow_to_image(flow),
                           "torch": lambda: torch_flow_to_image(flow, wheel),
                           "fused_img_only": lambda: flow_vis.flow_to_image(flow, anglemap=False),
                           "fused_given_radii": lambda: flow_vis.flow_to_image(flow, maxrad=radii)}, iters, warmup)
    npix = B * H * W
    nbytes = {"fused": 22.0, "torch": 22.0, "fused_img_only": 19.0, "fused_given_radii": 14.0}
    rows = {k: {"us": round(v, 1), "alg_bytes": int(nbytes[k] * npix), "frac_8TBs": round(nbytes[k] * npix / (v * 1e-6) / 1e9 / PEAK_GBS, 4)}
            for k, v in us.items()}
    rows["fused"]["x_torch"] = round(us["fused"] / us["torch"], 4)
    return {"batch": B, "height": H, "width": W, "bytes_equal_to_torch": agree, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_flowvis.py needs a GPU")
    result = {"bench": "flow_to_image", "iters": args.iters, "device": torch.cuda.get_device_name(0),
              "cases": [case_rows(B, H, W, args.iters, args.warmup) for B, H, W in CASES]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
