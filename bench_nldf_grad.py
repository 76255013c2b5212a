#!/usr/bin/env python3
"""NLDF's training step at 1 x 352 x 352, synthetic weights: per mode the median time over HIP events (>= 20 timed calls after
warm-up), the calls taking turns so that clock and cache state are shared:
  build_model        trunk + head forward;
  loss               build_model + build_loss;
  pools_grad         ... + the head walk to the five pools (trunk frozen, no variable gradients);
  pools_grad_w       ... + the head walk with the 30 variable gradients;
  backward_full      ... + Model.backward with head and trunk variable gradients and the input gradient;
  torch_head         the same head built from torch ops on the same device, forward + backward from the same Score gradient to the pools
                     and the 30 variables (the trunk excluded), to compare against head_fwd_bwd = the head's share of pools_grad_w;
and, called alone through the C ABI, the launches of the two 176 x 176 layers of the walk (Local_Fea: dgrad + wgrad; Fea_P2_Deconv:
the stride-2 convolution that is its input gradient + wgrad).  Prints one JSON line.  Not part of bench.py's workload."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_vgg_grad import time_interleaved   # noqa: E402
from coupe.optical_flow_based_deep_video_stabilization_amd import NLDF, runtime   # noqa: E402

B = 1


def torch_head(pools, w):
    """The head of NLDF.py:36-77 from torch ops (NCHW inside): Score [B,176,176,2]."""
    nchw = lambda t: t.permute(0, 3, 1, 2)
    conv = lambda t, n, pad: F.conv2d(t, w[n + "/W"].permute(3, 2, 0, 1), w[n + "/b"], padding=pad)
    contrast = lambda t: t - F.avg_pool2d(F.pad(t, (1, 1, 1, 1), mode="replicate"), 3, 1)
    p = [nchw(t) for t in pools]
    fg = conv(torch.relu(conv(torch.relu(conv(p[4], "Fea_Global_1", 0)), "Fea_Global_2", 0)), "Fea_Global", 0)
    P = [torch.relu(conv(p[k], f"Fea_P{k + 1}", 1)) for k in range(5)]
    cat = torch.cat([P[4], contrast(P[4])], 1)
    for k in (3, 2, 1, 0):
        n = f"Fea_P{k + 2}_Deconv"
        h = P[k].shape[2]
        up = F.conv_transpose2d(cat, w[n + "/W"].permute(3, 2, 0, 1), w[n + "/b"], stride=2, padding=1)[:, :, :h, :h]
        cat = torch.cat([P[k], contrast(P[k]), torch.relu(up)], 1)
    score = conv(conv(cat, "Local_Fea", 0), "Local_Score", 0) + conv(fg, "Global_Score", 0)
    return score.permute(0, 2, 3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_nldf_grad.py needs a GPU")
    g = torch.Generator().manual_seed(3)
    x = torch.rand(B, 352, 352, 3, generator=g).cuda()
    label = torch.zeros(B, 176, 176, 2)
    label[:, 40:120, 50:140, 0] = 1.0
    label[..., 1] = 1.0 - label[..., 0]
    label = label.cuda()
    hw = NLDF.synthetic_head_weights(seed=6, gain=1.2)
    m = NLDF.Model(seed=7, head_weights=hw)
    m.vgg.reuse_outputs = True

    def fwd():
        m.build_model(x, B)

    def loss():
        fwd()
        m.build_loss(label)

    def pools_grad(w):
        def run():
            loss()
            m.pools_grad(need_head_weights=w)
        return run

    def full():
        loss()
        m.backward(need_input=True, need_trunk_weights=True, need_head_weights=True)

    loss()
    dscore = m.Score_grad.clone()
    pools = [t.detach().clone().requires_grad_(True) for t in m._last["pools"]]
    tw = {k: torch.from_numpy(v).cuda().requires_grad_(True) for k, v in hw.items()}
    leaves = pools + list(tw.values())

    def torch_fwd_bwd():
        torch.autograd.grad(torch_head(pools, tw), leaves, dscore)

    # the two 176 x 176 layers alone, on the buffers of a real walk
    dev = x.device
    cat1, cat2 = m.internals()["cat1"], m.internals()["cat2"]
    dlf, dcat1 = torch.randn(B, 176, 176, 640, device=dev), torch.randn(B, 176, 176, 768, device=dev)
    dcat2 = torch.empty(B, 88, 88, 640, device=dev)
    W_lf, W_d2 = tw["Local_Fea/W"].detach(), tw["Fea_P2_Deconv/W"].detach()
    dW_lf, db_lf, dW_d2 = torch.empty_like(W_lf), torch.empty(640, device=dev), torch.empty_like(W_d2)
    ws = {"lf_dgrad": runtime.workspace(dev, "vstab_conv_dgrad_workspace_bytes", B, 176, 176, 640, 640, 1, 1, 0, 176, 176, 768, 0, 768, 0),
          "lf_wgrad": runtime.workspace(dev, "vstab_conv_wgrad_workspace_bytes", B, 176, 176, 1, 768, 640),      # covers a piece's too
          "d2_dgrad": runtime.workspace(dev, "vstab_conv_forward_workspace_bytes", B, 176, 176, 768, 512, 5, 2, 1, 640, 640, 0, 0, 88, 88),
          "d2_wgrad": runtime.workspace(dev, "vstab_conv_wgrad_workspace_bytes", B, 88, 88, 5, 512, 640)}
    layer = {
        "Local_Fea_dgrad": lambda: runtime.call(dev, "vstab_conv_dgrad", dlf.data_ptr(), B, 176, 176, 640, 0, 640, W_lf.data_ptr(), None, 1, 1, 0,
                                                dcat1.data_ptr(), 176, 176, 768, 0, 768, 0, ws["lf_dgrad"].data_ptr(), ws["lf_dgrad"].numel()),
        "Local_Fea_wgrad": lambda: runtime.call(dev, "vstab_conv_wgrad", cat1.data_ptr(), B, 176, 176, 768, 0, 768, dlf.data_ptr(), 176, 176, 640, 0, 640,
                                                1, 1, 0, dW_lf.data_ptr(), db_lf.data_ptr(), 0, ws["lf_wgrad"].data_ptr(), ws["lf_wgrad"].numel()),
        # the walk's form of the same filter gradient: eight row pieces of a sample that add into dW
        "Local_Fea_wgrad_8_pieces": lambda: [runtime.call(dev, "vstab_conv_wgrad", cat1.data_ptr() + c * 3872 * 768 * 4, 1, 3872, 1, 768, 0, 768,
                                                          dlf.data_ptr() + c * 3872 * 640 * 4, 3872, 1, 640, 0, 640, 1, 1, 0, dW_lf.data_ptr(), None,
                                                          1 if c else 0, ws["lf_wgrad"].data_ptr(), ws["lf_wgrad"].numel()) for c in range(8)],
        "Fea_P2_Deconv_dgrad": lambda: runtime.call(dev, "vstab_conv_forward", dcat1.data_ptr(), B, 176, 176, 768, 256, 512, W_d2.data_ptr(), None, 5, 2, 1,
                                                    dcat2.data_ptr(), 88, 88, 640, 0, 640, 0, ws["d2_dgrad"].data_ptr(), ws["d2_dgrad"].numel()),
        "Fea_P2_Deconv_wgrad": lambda: runtime.call(dev, "vstab_conv_wgrad", dcat1.data_ptr(), B, 176, 176, 768, 256, 512, cat2.data_ptr(), 88, 88, 640, 0,
                                                    640, 5, 2, 1, dW_d2.data_ptr(), None, 0, ws["d2_wgrad"].data_ptr(), ws["d2_wgrad"].numel()),
    }
    fns = {"build_model": fwd, "loss": loss, "pools_grad": pools_grad(False), "pools_grad_w": pools_grad(True), "backward_full": full,
           "torch_head": torch_fwd_bwd}
    fns.update(layer)
    us = time_interleaved(fns, args.iters, args.warmup)
    # the head alone, forward + backward: the forward's head share is build_model minus the trunk, measured the same way
    trunk_us = time_interleaved({"trunk": lambda: m.vgg.build(m._last["vgg"]["x"])}, args.iters, args.warmup)["trunk"]
    us["trunk_forward"] = trunk_us
    us["head_fwd_bwd"] = us["pools_grad_w"] - us["loss"] + us["build_model"] - trunk_us
    walk = us["pools_grad_w"] - us["loss"]
    in_walk = ("Local_Fea_dgrad", "Local_Fea_wgrad_8_pieces", "Fea_P2_Deconv_dgrad", "Fea_P2_Deconv_wgrad")
    share = sum(us[k] for k in in_walk) / walk if walk > 0 else None
    print(json.dumps({"bench": "nldf_forward_backward", "batch": B, "height": 352, "width": 352, "iters": args.iters,
                      "device": torch.cuda.get_device_name(0), "us": {k: round(v, 1) for k, v in us.items()},
                      "head_walk_us": round(walk, 1), "share_of_walk_in_176x176_layers": round(share, 3) if share is not None else None}))


if __name__ == "__main__":
    main()
