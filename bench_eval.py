#!/usr/bin/env python3
"""The test pass of the training loop (main:277-326, 431-441): `Trainer.evaluate` -- test-mode forward on the training graph's own
variables + the loss report -- against the two ways the same number could be had before it existed.  One JSON line.

    python bench_eval.py [--shapes 8x512x512,8x384x512 --evals 10 --rounds 5 --warmup 3]

Variants, each one evaluation of `loss_main_test` on a batch:
    evaluate            Trainer.evaluate(feats, gtstab, unstab)                       (no previews)
    evaluate_u8         ... previews='uint8'                                          (the image log's warpedimg2..6 as well)
    train_forward       Trainer.forward + loss_main_fused without gradients           (BatchNorm on BATCH statistics: not the same
                                                                                       number, and it moves the moving averages)
    sync_inference      sync_to_inference(trainer) + flownetS_pyramid(is_train=False) + loss_main_fused, the sync counted: every
                        variable through host memory, BatchNorm re-folded, weights re-packed

Method: every variant is warmed up at every shape; then `rounds` rounds, each timing every variant once, in turn (so that drift and
other tenants of the machine hit all of them alike), a timing being one untimed call and then a host clock around `evals` evaluations
that ends in a device synchronise (sync_inference: one evaluation per timing, its host work is the cost).  Reported: the median
over the rounds in ms per evaluation, and the spread (min, max); and the two test-mode values of loss_main_test, taken on the same
variables before anything moves the moving statistics again, with their difference.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="8x512x512,8x384x512", help="comma-separated BxHxW")
    ap.add_argument("--evals", type=int, default=10, help="evaluations per timing")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-sync-inference", action="store_true", help="leave the host round trip out (it dominates the run time)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py needs a GPU")
    torch.cuda.set_device(0)
    from coupe.optical_flow_based_deep_video_stabilization_amd import model, runtime, train_step, training, weights as wts

    result = {"metric": "ms per evaluation of loss_main_test (median over rounds; min, max)", "evals_per_timing": args.evals,
              "rounds": args.rounds, "shapes": {}}
    for shape in args.shapes.split(","):
        B, H, W = (int(v) for v in shape.split("x"))
        runtime.reset()
        w = wts.synthetic_weights(seed=1, cin=27, random_bn=True, flow_gain=0.5)
        g = torch.Generator().manual_seed(0)
        feats = torch.rand(B, H, W, 27, generator=g).cuda()
        gt, un = torch.rand(B, H, W, 3, generator=g).cuda(), torch.rand(B, H, W, 3, generator=g).cuda()
        tr = train_step.Trainer(w, B, H, W)
        tr.step(feats, gt, un, 1e-4)                      # the state a test pass meets: after training steps

        def sync_inference():
            train_step.sync_to_inference(tr)
            return training.loss_main_fused(model.flownetS_pyramid(feats, B, is_train=False), gt, un)

        variants = {
            "evaluate": lambda: tr.evaluate(feats, gt, un).total,
            "evaluate_u8": lambda: tr.evaluate(feats, gt, un, previews="uint8").total,
            "train_forward": lambda: (tr.forward(feats), training.loss_main_fused(tr.pf, gt, un))[1],
        }
        if not args.no_sync_inference:
            variants["sync_inference"] = sync_inference
        # the two test-mode numbers on the SAME variables, before any train-mode forward moves the moving statistics again
        values = {"evaluate": float(tr.evaluate(feats, gt, un).total)}
        if not args.no_sync_inference:
            values["sync_inference"] = float(sync_inference())
        values["train_forward"] = float(variants["train_forward"]())
        for name, fn in variants.items():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        times = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                n = 1 if name == "sync_inference" else args.evals
                if n > 1:
                    fn()                                  # untimed: the variant before it left caches and clocks in its own state
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _k in range(n):
                    fn()
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / n)
        entry = {name: {"ms": round(statistics.median(t), 3), "min": round(min(t), 3), "max": round(max(t), 3)} for name, t in times.items()}
        # the test-mode numbers must agree (same variables, same statistics); the train-mode one is a different number
        entry["loss_main_test"] = float(values["evaluate"])
        if "sync_inference" in values:
            entry["sync_inference_minus_evaluate"] = float(values["sync_inference"]) - float(values["evaluate"])
        entry["loss_main_train_mode"] = float(values["train_forward"])
        result["shapes"][shape] = entry
        del tr
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
