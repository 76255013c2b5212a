#!/usr/bin/env python3
"""NLDF's fused saliency loss with its gradient to Score (NLDF.saliency_loss + backward: three launches) at [8,176,176,2], the size
NLDF.Model runs it at with a batch of 8, against a torch composition of the same arithmetic (softmax, replicate pad, depthwise conv2d,
sqrt, tanh, the IoU and cross-entropy reductions, and autograd for the gradient).  Median time over HIP events of interleaved calls
(A B A B ...) after warm-up; the two results are compared on the same seeded input before anything is timed.  The tensors are small
(248 KB per sample): both sides are bound by launch latency, not bandwidth, so what the figures show is the cost of about fifty
launches against three.  It is a comparison, not a gate.  Prints one JSON line.  Not part of bench.py's workload."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coupe.optical_flow_based_deep_video_stabilization_amd import NLDF   # noqa: E402

B, H, W = 8, 176, 176


def time_interleaved(fns, iters, warmup):
    """median us of each call, the calls taking turns so that clock and cache state are shared"""
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


def torch_im_gradient(x, fx, fy):
    """x [B,H,W,2] -> [B,H,W,2]"""
    xp = F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1), mode="replicate")
    gx, gy = F.conv2d(xp, fx, groups=2), F.conv2d(xp, fy, groups=2)
    return torch.sqrt(gx * gx + gy * gy).permute(0, 2, 3, 1)


def torch_loss(score, label, fx, fy, th=1.5):
    pg = torch.tanh(torch_im_gradient(torch.softmax(score, dim=-1), fx, fy).sum(dim=-1, keepdim=True))
    lg = (torch_im_gradient(label, fx, fy).sum(dim=-1, keepdim=True) > th).float()
    iou = 1 - 2 * ((pg * lg).sum() + 1) / ((pg * pg).sum() + (lg * lg).sum() + 1)
    return iou + (-(label * torch.log_softmax(score, dim=-1)).sum(dim=-1)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_nldf_loss.py needs a GPU")
    g = torch.Generator().manual_seed(176)
    score = (torch.randn(B, H, W, 2, generator=g) * 3.0).cuda()
    a = torch.zeros(B, H, W)
    for n in range(B):                                   # one-hot labels: a rectangle per sample
        a[n, 20 + 5 * n:120 + 3 * n, 30 + 4 * n:140 - 2 * n] = 1.0
    label = torch.stack((a, 1.0 - a), dim=-1).cuda()
    k = torch.tensor([[-1., 0., 1.], [-2., 0., 2.], [-1., 0., 1.]])
    fx, fy = k.expand(2, 1, 3, 3).contiguous().cuda(), k.t().expand(2, 1, 3, 3).contiguous().cuda()
    sg, st = score.clone().requires_grad_(True), score.clone().requires_grad_(True)

    def fused():
        return torch.autograd.grad(NLDF.saliency_loss(sg, label).Loss_Mean, sg)[0]

    def fused_raw():
        return NLDF.nldf_loss.saliency_loss_call(score, label, 1.5, False, True)[3]

    def composed():
        return torch.autograd.grad(torch_loss(st, label, fx, fy), st)[0]

    value, tvalue = float(NLDF.saliency_loss(score, label).Loss_Mean), float(torch_loss(score, label, fx, fy))
    gdiff = float((fused() - composed()).abs().max())
    gmax = float(composed().abs().max())
    us = time_interleaved({"fused_autograd": fused, "fused_raw_entry": fused_raw, "torch_composition": composed}, args.iters, args.warmup)
    print(json.dumps({"bench": "nldf_saliency_loss_with_dscore", "batch": B, "height": H, "width": W, "iters": args.iters,
                      "device": torch.cuda.get_device_name(0), "launches_fused": 3, "value": value, "torch_value": tvalue,
                      "dscore_max_abs_diff": gdiff, "dscore_max_abs": gmax, "us": {k: round(v, 1) for k, v in us.items()},
                      "x_torch": round(us["fused_autograd"] / us["torch_composition"], 4)}))


if __name__ == "__main__":
    main()
