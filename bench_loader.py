#!/usr/bin/env python3
"""data_loader.Data_Loader at the reference's training shape: one batch of B = 8 at 384 x 512 assembled on the device from resident
720p uint8 clips (`vstab_assemble_train_batch`: resize + layout of feats [8,384,512,27], gtstab and unstab [8,384,512,3]), against
the same batch delivered the only way possible without it: an asynchronous copy of the finished fp32 tensors (189 MB) from pinned
host memory.  The copy's side does not count the host's ten cv2.resize calls per sample; it is the floor of what a host-built batch
costs.  The calls take turns (A B C A B C ...) and are timed with HIP events, median over >= 20 calls after warm-up.

Per row: the bytes that have to be WRITTEN (30 floats per output pixel; 27 for the yardstick), per second, as a share of 8 TB/s.
The yardstick is `vstab_assemble_input`, the inference side's assembly at the same output size (no resize, 27 planes), in the same
run.  `loader_batch` is `feed_the_network()` as a user calls it (plan bookkeeping, index arrays and one launch per clip present).
Prints one JSON line.  Not part of bench.py's workload."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, data_loader, runtime   # noqa: E402

PEAK_GBS = 8000.0
SKIP = [1, 9, 17, 25, 28, 29, 30, 31, 32]
B, H, W, SH, SW = 8, 384, 512, 720, 1280
CLIPS, FRAMES = 2, 40


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    if args.iters < 20:
        ap.error("--iters must be >= 20")
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader.py needs a GPU")
    g = torch.Generator(device="cuda").manual_seed(0)
    clip = lambda: torch.randint(0, 256, (FRAMES, SH, SW, 3), dtype=torch.uint8, device="cuda", generator=g)      # noqa: E731
    stab, unstab = [clip() for _ in range(CLIPS)], [clip() for _ in range(CLIPS)]
    loader = data_loader.Data_Loader.from_clips(SKIP, stab, unstab, H, W, B, True, rng=np.random.RandomState(0))
    loader.init_data_loader()

    def loader_batch():
        feed, is_end, _ = loader.feed_the_network()
        if is_end:                                   # the request that ends an epoch assembles nothing: ask again
            loader.feed_the_network()

    # the kernel alone: one fixed batch of one clip, eight samples at different offsets = one launch
    L = _lib.lib()
    out = [torch.empty((B, H, W, c), dtype=torch.float32, device="cuda") for c in (27, 3, 3)]
    rows = np.arange(B, dtype=np.int32)
    fidx = np.ascontiguousarray(np.arange(B, dtype=np.int32)[:, None] + np.asarray(SKIP, np.int32)[None, :])
    s0, u0 = loader.stab_clips[0], loader.unstab_clips[0]

    def kernel_batch():
        _lib.check(L.vstab_assemble_train_batch(s0.data_ptr(), u0.data_ptr(), FRAMES, SH, SW, rows.ctypes.data_as(_lib.c_int32_p),
                                                fidx.ctypes.data_as(_lib.c_int32_p), B, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                B, H, W, runtime.stream_ptr()))

    # what it replaces: the finished fp32 batch copied from pinned host memory
    host = [torch.rand((B, H, W, c), dtype=torch.float32).pin_memory() for c in (27, 3, 3)]
    dev = [torch.empty_like(t, device="cuda") for t in host]

    def pinned_copy():
        for d, h in zip(dev, host):
            d.copy_(h, non_blocking=True)

    # the yardstick: the inference side's assembly at the same output size
    slots = [torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(9)]
    ptrs = (C.c_void_p * 9)(*[t.data_ptr() for t in slots])
    feats_inf = torch.empty((B, H, W, 27), dtype=torch.float32, device="cuda")

    def assemble_input():
        _lib.check(L.vstab_assemble_input(ptrs, B, H, W, feats_inf.data_ptr(), runtime.stream_ptr()))

    us = time_interleaved({"kernel_batch": kernel_batch, "loader_batch": loader_batch, "pinned_copy": pinned_copy,
                           "assemble_input": assemble_input}, args.iters, args.warmup)
    npix = B * H * W
    written = {"kernel_batch": 120 * npix, "loader_batch": 120 * npix, "pinned_copy": 120 * npix, "assemble_input": 108 * npix}
    rows_out = {k: {"us": round(v, 1), "bytes_written": written[k], "GBs": round(written[k] / (v * 1e-6) / 1e9, 1),
                    "frac_8TBs": round(written[k] / (v * 1e-6) / 1e9 / PEAK_GBS, 4)} for k, v in us.items()}
    result = {"bench": "data_loader_batch", "batch": B, "height": H, "width": W, "source": [SH, SW], "clips": CLIPS, "frames_per_clip": FRAMES,
              "iters": args.iters, "device": torch.cuda.get_device_name(0), "rows": rows_out,
              "device_assembly_x_pinned_copy": round(us["pinned_copy"] / us["loader_batch"], 2),
              "faster_than_pinned_copy": bool(us["loader_batch"] < us["pinned_copy"]),
              "kernel_x_assemble_input_bandwidth": round(rows_out["kernel_batch"]["GBs"] / rows_out["assemble_input"]["GBs"], 3)}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
