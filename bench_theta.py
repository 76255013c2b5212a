#!/usr/bin/env python3
"""The theta regressors (model.flownetS_prehomo, model.Localizer) and their dense kernel alone: flownetS_prehomo at B = 1 and 8 on
384 x 512 x 27, Localizer at B = 8 on 256 x 256 x 3, vstab_dense_forward at (B, K, N) = (8, 393216, 256).  Per case the median time over
HIP events (>= 20 timed calls after warm-up), interleaved with a composition of torch ops on the GPU that does the same arithmetic
(NCHW conv2d on a replicate-padded input -- SYMMETRIC by one pixel is replicate --, eval-mode batch_norm, leaky_relu, max_pool2d with
ceil_mode, addmm); that is a comparison, not a gate.  The dense kernel's bytes are what the layer has to move: W once, x once, y once
(the slab partial sums it also writes and reads are its own overhead and are not counted), over its time, next to the 8 TB/s the project
quotes.  Synthetic weights with random BatchNorm statistics.  Prints one JSON line.  Not part of bench.py's workload."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import coupe.optical_flow_based_deep_video_stabilization_amd as vs   # noqa: E402
from coupe.optical_flow_based_deep_video_stabilization_amd import runtime, theta_nets, theta_runtime   # noqa: E402

PEAK_GBS = 8000.0
DENSE_CASE = (8, 393216, 256)


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


class TorchNet:
    """the graph of theta_nets.graph(net) from torch ops, NCHW, on the same variables"""

    def __init__(self, net, w, last_act="identity"):
        self.g, self.last_act = theta_nets.graph(net), last_act
        self.p = {k: torch.from_numpy(v).cuda() for k, v in w.items() if k in self.g.live_names(w)}
        for st in self.g.convs:
            self.p[st.name + "/W_conv2d"] = self.p[st.name + "/W_conv2d"].permute(3, 2, 0, 1).contiguous()
        self.scale = torch.tensor(theta_nets.HOMO_SCALE, device="cuda")
        self.shift = torch.tensor(theta_nets.HOMO_SHIFT, device="cuda")

    def _bn(self, x, name):
        p = self.p
        return F.leaky_relu(F.batch_norm(x, p[name + "/moving_mean"], p[name + "/moving_variance"], None, p[name + "/beta"], False, 0.0,
                                         theta_nets.BN_EPS), theta_nets.LRELU_SLOPE)

    def _act(self, u, act):
        if act == "lrelu":
            return F.leaky_relu(u, theta_nets.LRELU_SLOPE)
        if act == "tanh":
            return torch.tanh(u)
        if act == "tanh_affine":
            return torch.tanh(u / 1000) * self.scale + self.shift
        return u

    @torch.no_grad()
    def __call__(self, feats):
        p, x = self.p, feats.permute(0, 3, 1, 2)
        for st in self.g.convs:
            if st.sym_pad:
                x = F.pad(x, (1, 1, 1, 1), mode="replicate")
            x = self._bn(F.conv2d(x, p[st.name + "/W_conv2d"], p[st.name + "/b_conv2d"], stride=st.stride), st.bn)
            if st.pool:
                x = F.max_pool2d(x, 2, 2, ceil_mode=True)
        x = x.permute(0, 2, 3, 1).reshape(x.shape[0], -1)
        for i, d in enumerate(self.g.dense):
            act = self.last_act if i == len(self.g.dense) - 1 and d.units is None else d.act
            x = self._act(torch.addmm(p[d.name + "/b"], x, p[d.name + "/W"]), act)
            if d.bn:
                x = self._bn(x, d.bn)
        return x


def net_case(net, B, H, W, C, iters, warmup, opd=None):
    runtime.reset()
    w = vs.initialize_global_variables(seed=1, cin=C, random_bn=True, net=net, H=H, W=W, out_param_dim=opd, dense_std=0.01)
    feats = torch.rand(B, H, W, C, generator=torch.Generator().manual_seed(B)).cuda()
    tnet = TorchNet(net, w)
    fn = (lambda: vs.Localizer(feats, opd)) if net == "Localizer" else (lambda: vs.flownetS_prehomo(feats, B))
    got, want = fn(), tnet(feats)
    us = time_interleaved({"hip": fn, "torch": lambda: tnet(feats)}, iters, warmup)
    return {"net": net, "batch": B, "height": H, "width": W, "channels": C, "us": round(us["hip"], 1), "torch_us": round(us["torch"], 1),
            "x_torch": round(us["hip"] / us["torch"], 3),
            "max_abs_diff_vs_torch": float((got - want).abs().max()), "max_abs_theta": float(want.abs().max())}


def dense_case(iters, warmup):
    B, K, N = DENSE_CASE
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, K, device="cuda", generator=g)
    W = torch.randn(K, N, device="cuda", generator=g) / K ** 0.5
    b = torch.randn(N, device="cuda", generator=g)
    got, want = theta_runtime.dense_forward(x, W, b, "lrelu"), F.leaky_relu(torch.addmm(b, x, W), theta_nets.LRELU_SLOPE)
    us = time_interleaved({"hip": lambda: theta_runtime.dense_forward(x, W, b, "lrelu"),
                           "torch": lambda: F.leaky_relu(torch.addmm(b, x, W), theta_nets.LRELU_SLOPE)}, iters, warmup)
    nbytes = 4 * (K * N + B * K + B * N + N)
    ws = int(theta_runtime._lib.lib().vstab_dense_forward_workspace_bytes(B, K, N))
    return {"B": B, "K": K, "N": N, "us": round(us["hip"], 1), "torch_us": round(us["torch"], 1), "x_torch": round(us["hip"] / us["torch"], 3),
            "alg_bytes": nbytes, "partial_sum_bytes_written_and_read": 2 * ws, "bytes_per_s": round(nbytes / (us["hip"] * 1e-6), 1),
            "frac_8TBs": round(nbytes / (us["hip"] * 1e-6) / 1e9 / PEAK_GBS, 4),
            "torch_frac_8TBs": round(nbytes / (us["torch"] * 1e-6) / 1e9 / PEAK_GBS, 4), "max_abs_diff_vs_torch": float((got - want).abs().max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_theta.py needs a GPU")
    result = {"bench": "theta_regressors", "iters": args.iters, "device": torch.cuda.get_device_name(0), "peak_bytes_per_s": PEAK_GBS * 1e9,
              "dense": dense_case(args.iters, args.warmup),
              "nets": [net_case("flownetS_prehomo", 1, 384, 512, 27, args.iters, args.warmup),
                       net_case("flownetS_prehomo", 8, 384, 512, 27, args.iters, args.warmup),
                       net_case("Localizer", 8, 256, 256, 3, args.iters, args.warmup, opd=6)]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
