#!/usr/bin/env python3
"""cell.ConvLSTMCell and cell.ConvGRUCell at B = 8, 64 x 64, Cx = F = 256, k = 3 (the conv3_1 feature size of the 512 x 512 headline),
with and without normalize: per case the median time over HIP events (>= 20 timed calls after warm-up) of one step, of the stage
that follows the convolution(s) alone (the launches of csrc/cell_ops.hip on the step's own buffers), and of an 8-step run_sequence
per step.  The stage's algorithmic bytes -- LSTM: y (4 N) and c read, the three peepholes read once per sample, c', h' and the h
slice written; GRU: y (2 N), h twice and y2 read, r h, h' and the h slice written; N = B H W F floats -- are given as a fraction of
8 TB/s.  For scale the same arithmetic composed of torch ops on the same device (F.conv2d in NCHW plus the elementwise and
reduction ops) is timed interleaved with the library's calls; it is a comparison, not a gate.  Prints one JSON line.  Not part of
bench.py's workload.

--backward adds, per case, the training step of a cell built with differentiable=True: forward + backward of the 8-step run_sequence
(gradients to the inputs and every parameter; upstream gradients given for every output, and for the LSTM's final c), the
gate-backward launches alone (training.conv*_backward on one step's saved buffers, their output allocations included), and the same
8-step training step composed of torch ops under torch.autograd, timed interleaved; also the largest difference of the two input
gradients.  Without the flag the output is what it was."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, cell, training   # noqa: E402

PEAK_GBS = 8000.0
B, H, W, CX, FILTERS, K, T = 8, 64, 64, 256, 256, 3, 8


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


def _ln(v, gamma, beta):
    """v [B,F,H,W]"""
    mean = v.mean(dim=(1, 2, 3), keepdim=True)
    d = v - mean
    var = (d * d).mean(dim=(1, 2, 3), keepdim=True)
    return d * torch.rsqrt(var + 1e-12) * gamma.view(1, -1, 1, 1) + beta.view(1, -1, 1, 1)


def torch_lstm(x, c, h, w, normalize):
    """NCHW; w: tensors on the device, the kernel as OIHW, the peepholes as [F,H,W]"""
    y = F.conv2d(torch.cat([x, h], 1), w["kernel"], None if normalize else w["bias"], padding=K // 2)
    j, i, f, o = torch.split(y, FILTERS, 1)
    i = i + w["W_ci"] * c
    f = f + w["W_cf"] * c
    if normalize:
        j, i, f = (_ln(v, w[f"{n}/gamma"], w[f"{n}/beta"]) for v, n in ((j, "LayerNorm"), (i, "LayerNorm_1"), (f, "LayerNorm_2")))
    c = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    o = o + w["W_co"] * c
    if normalize:
        o, c = _ln(o, w["LayerNorm_3/gamma"], w["LayerNorm_3/beta"]), _ln(c, w["LayerNorm_4/gamma"], w["LayerNorm_4/beta"])
    return c, torch.sigmoid(o) * torch.tanh(c)


def torch_gru(x, h, w, normalize):
    y = F.conv2d(torch.cat([x, h], 1), w["gates/kernel"], None if normalize else w["gates/bias"], padding=K // 2)
    r, u = torch.split(y, FILTERS, 1)
    if normalize:
        r, u = _ln(r, w["gates/LayerNorm/gamma"], w["gates/LayerNorm/beta"]), _ln(u, w["gates/LayerNorm_1/gamma"], w["gates/LayerNorm_1/beta"])
    r, u = torch.sigmoid(r), torch.sigmoid(u)
    y2 = F.conv2d(torch.cat([x, r * h], 1), w["candidate/kernel"], None if normalize else w["candidate/bias"], padding=K // 2)
    if normalize:
        y2 = _ln(y2, w["candidate/LayerNorm/gamma"], w["candidate/LayerNorm/beta"])
    return u * h + (1 - u) * torch.tanh(y2)


def _torch_weights(w):
    out = {}
    for n, a in w.items():
        t = torch.from_numpy(a).cuda()
        if n.endswith("kernel"):
            t = t.permute(3, 2, 0, 1).contiguous()
        elif n.startswith("W_c"):
            t = t.permute(2, 0, 1).contiguous()
        out[n] = t
    return out


def backward_rows(kind, normalize, w, xs, iters, warmup):
    """the --backward columns of one case"""
    g = torch.Generator().manual_seed(29)
    lstm = kind == "lstm"
    cl = (cell.ConvLSTMCell if lstm else cell.ConvGRUCell)([H, W], FILTERS, [K, K], normalize=normalize, differentiable=True)
    cl.assign_weights(w)
    params = list(cl.parameters().values())
    gout = torch.randn(T, B, H, W, FILTERS, generator=g).cuda()
    gc = torch.randn(B, H, W, FILTERS, generator=g).cuda()
    xl = xs.clone().requires_grad_()

    def train():
        xl.grad = None
        for p in params:
            p.grad = None
        outs, final = cell.run_sequence(cl, xl)
        torch.autograd.backward([outs, final.c] if lstm else [outs], [gout, gc] if lstm else [gout])

    tw = {n: t.requires_grad_() for n, t in _torch_weights(w).items()}
    xt = xs.permute(0, 1, 4, 2, 3).contiguous().requires_grad_()
    gout_t, gc_t = gout.permute(0, 1, 4, 2, 3).contiguous(), gc.permute(0, 3, 1, 2).contiguous()

    def torch_train():
        xt.grad = None
        for p in tw.values():
            p.grad = None
        h = c = torch.zeros(B, FILTERS, H, W, device="cuda")
        outs = []
        for t in range(T):
            if lstm:
                c, h = torch_lstm(xt[t], c, h, tw, normalize)
            else:
                h = torch_gru(xt[t], h, tw, normalize)
            outs.append(h)
        torch.autograd.backward([torch.stack(outs), c] if lstm else [torch.stack(outs)], [gout_t, gc_t] if lstm else [gout_t])

    # one step's saved buffers for the gate backward alone
    with torch.no_grad():
        x0, z = xs[0], torch.zeros(B, H, W, FILTERS, device="cuda")
        cl.call(x0, (z, z) if lstm else z)
    bufs, L, dev = cl.buffers(B, xs.device), _lib.lib(), cl._dev
    dh = gout[0]
    if lstm:
        stats = tuple(cl._stats(bufs.gate_ws, int(L.vstab_convlstm_gates_stats_offset(B, H, W, FILTERS, q)), n, B)
                      for q, n in ((0, 3), (1, 2))) if normalize else None
        pe = tuple(dev[n] for n in ("W_ci", "W_cf", "W_co"))

        def gates():
            training.convlstm_gates_backward(bufs.y, z, dh, gc, pe, dev.get("gamma"), dev.get("beta"), stats)
    else:
        # (the update's statistics are in the workspace; the gates' were overwritten by them: a gates call puts them back)
        off = int(L.vstab_convgru_stats_offset(B, H, W, FILTERS))
        stats_c = cl._stats(bufs.gate_ws, off, 1, B) if normalize else None
        cl._gates(bufs)
        stats_g = cl._stats(bufs.gate_ws, off, 2, B) if normalize else None
        h_old, drh = bufs.cat2[..., cl._hoff:cl._hoff + FILTERS], gc

        def gates():
            du, _, dhh, _ = training.convgru_update_backward(bufs.y2, h_old, bufs.u, dh, dev.get("candidate/gamma"), dev.get("candidate/beta"), stats_c)
            training.convgru_gates_backward(bufs.y, h_old, du, drh, dhh, dev.get("gates/gamma"), dev.get("gates/beta"), stats_g)

    train()
    torch_train()
    diff = float((xl.grad.permute(0, 1, 4, 2, 3) - xt.grad).abs().max())
    us = time_interleaved({"train": train, "gates": gates, "torch_train": torch_train}, iters, warmup)
    return {"train_sequence8_us": round(us["train"], 1), "gate_backward_us": round(us["gates"], 1),
            "torch_train_sequence8_us": round(us["torch_train"], 1), "train_x_torch": round(us["train"] / us["torch_train"], 3),
            "max_abs_dinputs_diff_vs_torch": diff}


def case_rows(kind, normalize, iters, warmup, backward=False):
    g = torch.Generator().manual_seed(17)
    x, c, h = (torch.rand(B, H, W, n, generator=g).mul_(2).sub_(1).cuda() for n in (CX, FILTERS, FILTERS))
    xs = torch.rand(T, B, H, W, CX, generator=g).mul_(2).sub_(1).cuda()
    nchw = lambda t: t.permute(0, 3, 1, 2).contiguous()         # noqa: E731
    xt, ct, ht = nchw(x), nchw(c), nchw(h)
    n_el = B * H * W * FILTERS
    if kind == "lstm":
        cl = cell.ConvLSTMCell([H, W], FILTERS, [K, K], normalize=normalize)
        w = cl.synthetic_weights(3, CX, random_ln=True)
        cl.assign_weights(w)
        tw = _torch_weights(w)
        step = lambda: cl.call(x, (c, h))                         # noqa: E731
        bufs = cl.buffers(B, x.device)
        c_out, h_out = torch.empty_like(c), torch.empty_like(c)
        post = lambda: cl._gates(bufs, c, c_out, h_out)           # noqa: E731
        tstep = lambda: torch_lstm(xt, ct, ht, tw, normalize)     # noqa: E731
        got, want = cl.call(x, (c, h))[0], torch_lstm(xt, ct, ht, tw, normalize)[1]
        alg = 4 * (8 * n_el + 3 * H * W * FILTERS)
    else:
        cl = cell.ConvGRUCell([H, W], FILTERS, [K, K], normalize=normalize)
        w = cl.synthetic_weights(3, CX, random_ln=True)
        cl.assign_weights(w)
        tw = _torch_weights(w)
        step = lambda: cl.call(x, h)                              # noqa: E731
        bufs = cl.buffers(B, x.device)
        h_out = torch.empty_like(h)

        def post():
            cl._gates(bufs)
            cl._update(bufs, h_out)
        tstep = lambda: torch_gru(xt, ht, tw, normalize)          # noqa: E731
        got, want = cl.call(x, h)[0], torch_gru(xt, ht, tw, normalize)
        alg = 4 * 8 * n_el
    with torch.no_grad():
        diff = float((got.permute(0, 3, 1, 2) - want).abs().max())
        step()                                                   # (leaves a whole step's y, y2 and u in the buffers that `post` reads)
        us = time_interleaved({"step": step, "post_conv": post, "sequence8": lambda: cell.run_sequence(cl, xs), "torch_step": tstep},
                              iters, warmup)
    row = {"cell": kind, "normalize": normalize, "max_abs_diff_vs_torch": diff, "step_us": round(us["step"], 1),
            "post_conv_us": round(us["post_conv"], 1), "post_conv_alg_bytes": alg,
            "post_conv_frac_8TBs": round(alg / (us["post_conv"] * 1e-6) / 1e9 / PEAK_GBS, 4),
            "sequence8_us_per_step": round(us["sequence8"] / T, 1), "torch_step_us": round(us["torch_step"], 1),
            "step_x_torch": round(us["step"] / us["torch_step"], 3)}
    if backward:
        row.update(backward_rows(kind, normalize, w, xs, iters, warmup))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--backward", action="store_true", help="add the training step (forward + backward of the 8-step sequence) per case")
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_cell.py needs a GPU")
    result = {"bench": "conv_rnn_cells", "batch": B, "height": H, "width": W, "in_channels": CX, "filters": FILTERS, "kernel": K,
              "iters": args.iters, "device": torch.cuda.get_device_name(0),
              "cases": [case_rows(kind, norm, args.iters, args.warmup, args.backward) for kind in ("lstm", "gru") for norm in (True, False)]}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
