"""The refusal contract of the theta regressors' C entry points (csrc/theta_api.cpp), on the CPU: every malformed call below returns
before any HIP call with this code, judged in the order NULL buffer, shape, alignment, workspace.  The pointers are addresses inside a
small host buffer and are never dereferenced; no call here would be accepted (test_sampler_abi_refusals_cpu.py's method)."""
import ctypes as C

import numpy as np
import pytest

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib

SHAPE, ALIGN, NOMEM, STATE = -1, -2, -4, -6

_BUF = np.zeros(64, np.float64)
P = _BUF.ctypes.data + (-_BUF.ctypes.data) % 16          # 16-byte aligned
OFF4, OFF2 = "P+4", "P+2"

SIGNATURES = {
    "pad_symmetric": "x B H W C p y cs_y stream",
    "bn_lrelu_slope_inference": "zy rows cs c_off C beta moving_mean moving_var eps slope twice stream",
    "bn_lrelu_slope_pool_inference": "z B H W C beta moving_mean moving_var eps slope twice out stream",
    "dense_forward": "x B K N W b act slope scale shift y workspace workspace_bytes stream",
}
DEFAULTS = {
    "pad_symmetric": dict(B=1, H=5, W=6, C=3, p=1, cs_y=4, stream=None),
    "bn_lrelu_slope_inference": dict(rows=6, cs=8, c_off=4, C=4, eps=1e-5, slope=0.2, twice=0, stream=None),
    "bn_lrelu_slope_pool_inference": dict(B=1, H=5, W=6, C=4, eps=1e-5, slope=0.2, twice=1, stream=None),
    "dense_forward": dict(B=2, K=128, N=8, act=1, slope=0.2, workspace_bytes=128, stream=None),          # 2 slabs x 2 x 8 floats
}


def call(entry, **bad):
    L = _lib.lib()
    values = {**DEFAULTS[entry], **bad}
    fn = getattr(L, "vstab_" + entry)
    names = SIGNATURES[entry].split()
    assert set(bad) <= set(names) and len(names) == len(fn.argtypes)
    args = []
    for name in names:
        v = values.get(name, P)
        args.append({OFF4: P + 4, OFF2: P + 2}.get(v, v) if isinstance(v, str) else v)
    return fn(*args), L.vstab_last_error(None).decode()


def nulls(pointers):
    return [({p: 0}, STATE) for p in pointers.split()]


BN = "beta moving_mean moving_var"
TABLE = {
    "pad_symmetric": nulls("x y") + [
        (dict(B=0), SHAPE), (dict(H=0), SHAPE), (dict(W=0), SHAPE), (dict(C=0), SHAPE), (dict(p=-1), SHAPE), (dict(p=6), SHAPE),
        (dict(H=1, W=9, p=2), SHAPE), (dict(cs_y=2), SHAPE), (dict(C=6, cs_y=6), SHAPE), (dict(B=4, H=8190, W=8190, C=4, cs_y=8), SHAPE),
        (dict(y=OFF4), ALIGN), (dict(x=OFF2), ALIGN), (dict(x=0, B=0), STATE), (dict(B=0, y=OFF4), SHAPE)],
    "bn_lrelu_slope_inference": nulls("zy " + BN) + [
        (dict(rows=0), SHAPE), (dict(C=0), SHAPE), (dict(c_off=-4), SHAPE), (dict(c_off=8), SHAPE), (dict(C=6, cs=12), ALIGN), (dict(cs=10), ALIGN),
        (dict(c_off=2, C=4), ALIGN), (dict(zy=OFF4), ALIGN), (dict(beta=OFF4), ALIGN), (dict(moving_mean=OFF4), ALIGN),
        (dict(moving_var=OFF4), ALIGN), (dict(zy=0, rows=0), STATE), (dict(rows=0, zy=OFF4), SHAPE)],
    "bn_lrelu_slope_pool_inference": nulls("z out " + BN) + [
        (dict(B=0), SHAPE), (dict(H=0), SHAPE), (dict(W=0), SHAPE), (dict(C=0), SHAPE), (dict(B=2, H=32768, W=8192, C=4), SHAPE),
        (dict(C=6), ALIGN), (dict(z=OFF4), ALIGN), (dict(out=OFF4), ALIGN), (dict(beta=OFF4), ALIGN), (dict(out=0, C=6), STATE),
        (dict(H=0, C=6), SHAPE)],
    "dense_forward": nulls("x W b y") + [
        (dict(act=3, scale=0), STATE), (dict(act=3, shift=0), STATE), (dict(B=0), SHAPE), (dict(B=33), SHAPE), (dict(K=0), SHAPE),
        (dict(K=126), SHAPE), (dict(N=0), SHAPE), (dict(act=4), SHAPE), (dict(act=-1), SHAPE), (dict(K=1 << 30, N=1 << 10), SHAPE),
        (dict(x=OFF4), ALIGN), (dict(y=OFF4), ALIGN), (dict(W=OFF4), ALIGN), (dict(W=OFF2, N=7, workspace_bytes=112), ALIGN),
        (dict(workspace=0), NOMEM), (dict(workspace_bytes=127), NOMEM), (dict(workspace=OFF4), ALIGN),
        (dict(workspace=OFF4, workspace_bytes=127), NOMEM), (dict(x=OFF4, workspace_bytes=0), ALIGN), (dict(B=0, x=OFF4), SHAPE),
        (dict(y=0, B=0), STATE)],
}
ROWS = [(e, bad, code) for e, rows in TABLE.items() for bad, code in rows]


def test_every_entry_point_has_rows():
    theta = [n[len("vstab_"):] for n in _lib.EXPORTS
             if n in ("vstab_pad_symmetric", "vstab_dense_forward") or n.startswith("vstab_bn_lrelu_slope")]
    assert sorted(theta) == sorted(TABLE) == sorted(SIGNATURES)


@pytest.mark.parametrize("entry,bad,code", ROWS, ids=[f"{e}-{'+'.join(f'{k}={v}' for k, v in b.items())}" for e, b, _ in ROWS])
def test_refusal(entry, bad, code):
    rc, msg = call(entry, **bad)
    assert rc == code and msg.startswith(entry + ": ")


def test_scale_and_shift_are_optional_without_the_affine_tail():
    """NULL scale / shift are no fault for act 0..2: the call gets as far as the workspace check"""
    assert call("dense_forward", scale=0, shift=0, workspace_bytes=0)[0] == NOMEM


def test_dense_workspace_and_plan():
    L = _lib.lib()
    q = L.vstab_dense_forward_workspace_bytes
    assert q(2, 128, 8) == 128 and q(1, 4, 8) == 32 and q(8, 393216, 256) == 1024 * 8 * 256 * 4
    for bad in [(0, 128, 8), (33, 128, 8), (2, 0, 8), (2, 126, 8), (2, 128, 0), (2, 1 << 30, 1 << 10)]:
        assert q(*bad) == 0, bad
    rows, slabs = C.c_int32(), C.c_int32()

    def plan(K, N):
        assert L.vstab_host_dense_plan(K, N, C.byref(rows), C.byref(slabs)) == 0
        return rows.value, slabs.value

    # the reference's first dense layer: 1024 slabs of 384 rows, one per wavefront asked for; small layers keep 64-row slabs
    assert plan(393216, 256) == (384, 1024) and plan(40960, 256) == (64, 640) and plan(4, 8) == (64, 1) and plan(1920, 1000) == (64, 30)
    for K, N in [(4, 8), (128, 8), (256, 128), (1000, 1000), (1920, 1000), (40960, 256), (393216, 256), (393216, 1000), (24 * 32 * 512, 7)]:
        r, s = plan(K, N)
        assert r % 4 == 0 and (s - 1) * r < K <= s * r and s <= 1024
        for B in (1, 5, 32):
            assert q(B, K, N) == s * B * N * 4          # the cut does not depend on B
    assert L.vstab_host_dense_plan(126, 8, C.byref(rows), C.byref(slabs)) == SHAPE and (rows.value, slabs.value) == (0, 0)
    assert L.vstab_host_dense_plan(128, 8, None, C.byref(slabs)) == STATE
