#!/usr/bin/env python3
"""Plan identity of two builds of libvstab_hip.so (no GPU needed): every integer, byte count, packed float and return code of the
host-side plan views over a grid of problems must be equal.  usage: plan_identity.py OLD.so NEW.so"""
import ctypes as C
import itertools
import sys

import numpy as np


class WsEntry(C.Structure):
    _fields_ = [("name", C.c_char * 24), ("offset_bytes", C.c_int64), ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
                ("c", C.c_int32), ("c_stride", C.c_int32)]


def load(path):
    L = C.CDLL(path)
    for f in ("vstab_workspace_bytes", "vstab_vgg16_workspace_bytes", "vstab_nldf_workspace_bytes"):
        getattr(L, f).restype = C.c_size_t
    for f in ("vstab_host_pack_layer", "vstab_host_pack_wdec"):
        getattr(L, f).restype = C.c_longlong
    return L


def ints(n, call):
    buf = (C.c_int32 * n)(*([-7] * n))
    return (call(buf, n), tuple(buf))


def plan_values(L, B, H, W, Cin):
    ent = (WsEntry * 24)()
    out = [L.vstab_workspace_bytes(B, H, W, Cin), ints(20, lambda o, n: L.vstab_level_sizes(H, W, o)),
           (L.vstab_workspace_layout(B, H, W, Cin, ent, 24), bytes(ent))]
    for l in range(4):
        out.append(ints(128, lambda o, n: L.vstab_host_wdec_plan(B, H, W, Cin, l, o, n)))
    for flags, pb, layer in itertools.product((0, 1, 2, 4, 8, 16, 3), (0, 8, 32), range(19)):
        out.append(ints(160, lambda o, n: L.vstab_host_layer_plan_pinned(pb, C.c_uint(flags), B, H, W, Cin, layer, o, n)))
    if Cin == 27:
        out += [ints(54, lambda o, n: L.vstab_vgg16_shapes(H, W, o)), L.vstab_vgg16_workspace_bytes(B, H, W), L.vstab_nldf_workspace_bytes(B)]
    return out


def pack_values(L, rng):
    shapes = [(7, 2), (5, 64), (5, 128), (3, 256), (3, 256), (3, 512), (3, 512), (3, 512), (3, 512), (3, 1024)]
    couts = [64, 128, 256, 256, 512, 512, 512, 512, 1024, 1024, 512, 256, 128, 64]
    dcin = [1024, 1026, 770, 386]
    cap = 1 << 24
    wpk = np.empty(cap, np.float32)
    out = []
    fp, dp = C.POINTER(C.c_float), C.POINTER(C.c_double)
    for Cin, layer, scaled in itertools.product((27, 6), range(19), (False, True)):
        if layer < 10:
            k, ci = shapes[layer]
            n = k * k * (Cin if layer == 0 else ci) * couts[layer]
        else:
            n = 16 * couts[layer] * dcin[layer - 10] if layer < 14 else 9 * (194 if layer == 14 else dcin[layer - 15]) * 2
        Wt = rng.standard_normal(n).astype(np.float32)
        sc = rng.random(1024) + 0.5
        wpk.fill(np.nan)
        r = L.vstab_host_pack_layer(Cin, layer, Wt.ctypes.data_as(fp), sc.ctypes.data_as(dp) if scaled else None, wpk.ctypes.data_as(fp), cap)
        out.append((r, wpk[:max(r, 0) + 64].tobytes()))
        if 10 <= layer < 14:
            wpk.fill(np.nan)
            r = L.vstab_host_pack_wdec(layer - 10, Wt.ctypes.data_as(fp), sc.ctypes.data_as(dp) if scaled else None, wpk.ctypes.data_as(fp), cap)
            out.append((r, wpk[:max(r, 0) + 64].tobytes()))
            out.append((L.vstab_host_pack_wdec(layer - 10, Wt.ctypes.data_as(fp), None, wpk.ctypes.data_as(fp), 16), b""))
    return out


def count(v):
    if isinstance(v, (list, tuple)):
        return sum(count(x) for x in v)
    return len(v) // 4 if isinstance(v, bytes) else 1


def main():
    old, new = load(sys.argv[1]), load(sys.argv[2])
    total = diffs = 0
    grid = itertools.product((1, 2, 3, 8, 16, 32), ((52, 44), (88, 104), (256, 256), (384, 512), (512, 512), (720, 1280), (1080, 1920)), (27, 6))
    for B, (H, W), Cin in grid:
        a, b = plan_values(old, B, H, W, Cin), plan_values(new, B, H, W, Cin)
        total += count(a)
        diffs += sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
        if B == 32 and (H, W) == (1080, 1920):
            print(f"B=32 1080x1920 Cin={Cin}: layer_plan(conv1) rc {a[7][0]} / {b[7][0]} (the 2 GiB refusal), workspace_bytes {a[0]} / {b[0]} (one chunk)")
    a, b = pack_values(old, np.random.default_rng(5)), pack_values(new, np.random.default_rng(5))
    total += count(a)
    diffs += sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
    print(f"compared {total} values, {diffs} differences")
    return 1 if diffs else 0


if __name__ == "__main__":
    sys.exit(main())
