"""The refusal contract of the samplers' C entry points (csrc/sampler_api.cpp), on the CPU: every malformed call below returns
before any HIP call, with exactly this code and exactly this vstab_last_error text.  Where two faults coincide the rows pin which
one is judged first: the 2-D entry points and warp.py's judge pointers, then shape; the 3-D volume family judges shape first.
The expectations were recorded from the library before the entry points moved out of api.cpp; moving or restating a check must
leave every row as it is.

The pointers are addresses inside a small host buffer and are never dereferenced; no call here would be accepted."""
import ctypes as C

import numpy as np
import pytest

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib

SHAPE, ALIGN, NOMEM, STATE = -1, -2, -4, -6

_BUF = np.zeros(64, np.float64)
P = _BUF.ctypes.data
assert P % 8 == 0
MISALIGNED = "P+4"                        # the workspace at P + 4 (a name, so that the test ids hold no address)

# argument names of every entry point, in the C order; a name outside DEFAULTS is a pointer
SIGNATURES = {
    "st_transform": "img B H W C theta theta_dim out oh ow stream",
    "st_transform_interp": "img B H W C theta theta_dim interp out oh ow stream",
    "st_bilinear_interp": "img B H W C x y oh ow out stream",
    "st_bicubic_interp": "img B H W C x y oh ow out stream",
    "st_meshgrid": "out oh ow stream",
    "st_symmetry_transform": "img B H W C theta kind interp out oh ow stream",
    "st_symmetry_matrix": "theta B kind out stream",
    "st_symmetry_coords": "theta B kind oh ow x_out y_out stream",
    "host_tps_linv": "g linv_t cap",
    "st_elastic_transform": "img B H W C theta g linv_t interp out oh ow stream",
    "st_elastic_coords": "theta B g linv_t oh ow x_out y_out stream",
    "st_transform_backward": "img B H W C theta theta_dim dout oh ow d_img accumulate d_theta workspace workspace_bytes stream",
    "st_transform_interp_backward": "img B H W C theta theta_dim interp dout oh ow d_img accumulate d_theta workspace workspace_bytes stream",
    "st_bilinear_interp_backward": "img B H W C x y dout oh ow d_img accumulate d_x d_y stream",
    "st_bicubic_interp_backward": "img B H W C x y dout oh ow d_img accumulate d_x d_y stream",
    "st_symmetry_transform_backward": "img B H W C theta kind dout oh ow d_img accumulate d_theta workspace workspace_bytes stream",
    "st_symmetry_transform_interp_backward": "img B H W C theta kind interp dout oh ow d_img accumulate d_theta workspace workspace_bytes stream",
    "st_elastic_transform_backward": "img B H W C theta g linv_t dout oh ow d_img accumulate d_theta workspace workspace_bytes stream",
    "st_elastic_transform_interp_backward": "img B H W C theta g linv_t interp dout oh ow d_img accumulate d_theta workspace workspace_bytes stream",
    "st3d_meshgrid": "out od oh ow stream",
    "st3d_bilinear_interp": "vol B D H W C x y z od oh ow edge_size out stream",
    "st3d_transform": "vol B D H W C theta out od oh ow stream",
    "st3d_transform_backward": "vol B D H W C theta dout od oh ow d_vol accumulate d_theta workspace workspace_bytes stream",
    "st3d_bilinear_interp_backward": "vol B D H W C x y z od oh ow edge_size dout d_vol accumulate dx dy dz stream",
    "homography_warp": "img B H W C M out oh ow stream",
    "transform_image": "img B H W C ref pM out oh ow stream",
    "vec2mtrx": "p B dim warp_approx out stream",
    "homography_warp_backward": "img B H W C M dout oh ow d_img accumulate d_M workspace workspace_bytes stream",
    "transform_image_backward": "img B H W C ref pM dout oh ow d_img accumulate d_pM workspace workspace_bytes stream",
    "vec2mtrx_backward": "p B dim warp_approx d_out d_p stream",
}

# a small well-formed call: 1x8x9x3 -> 6x7 (the volume: 1x4x5x6x2 -> 3x4x5); the symmetric-pad family needs H, W >= 100
DEFAULTS = dict(B=1, H=8, W=9, C=3, oh=6, ow=7, D=4, od=3, theta_dim=6, interp=0, kind=0, g=2, cap=28, accumulate=0, edge_size=1, dim=8,
                warp_approx=4, stream=None)
VOLUME = dict(H=5, W=6, C=2, oh=4, ow=5)
SYMMETRIC = dict(H=104, W=117)

# workspace bytes of the well-formed call of each backward with a parameter gradient (also what its size query answers, below)
WORKSPACE = {
    "st_transform_backward": 64,
    "st_transform_interp_backward": 64,
    "st_symmetry_transform_backward": 128,
    "st_symmetry_transform_interp_backward": 128,
    "st_elastic_transform_backward": 112,
    "st_elastic_transform_interp_backward": 112,
    "st3d_transform_backward": 192,
    "homography_warp_backward": 72,
    "transform_image_backward": 72,
}


def call(entry, **bad):
    """The well-formed call of `entry` with the arguments in `bad` replaced -> (return code, vstab_last_error)."""
    L = _lib.lib()
    values = dict(DEFAULTS)
    if entry.startswith("st3d"):
        values.update(VOLUME)
    if entry.startswith("st_symmetry"):
        values.update(SYMMETRIC)
    values["workspace_bytes"] = WORKSPACE.get(entry, 0)
    names = SIGNATURES[entry].split()
    assert set(bad) <= set(names), (entry, bad)
    values.update(bad)
    fn = getattr(L, "vstab_" + entry)
    args = []
    for name, ctype in zip(names, fn.argtypes):
        v = values.get(name, P)
        if v == MISALIGNED:
            v = P + 4
        if ctype is _lib.c_float_p:
            v = C.cast(v, _lib.c_float_p)
        args.append(v)
    assert len(args) == len(fn.argtypes)
    rc = fn(*args)
    return rc, L.vstab_last_error(None).decode()


def nulls(pointers, code, tail):
    return [({p: 0}, code, tail) for p in pointers.split()]


BIG = dict(H=32768, W=32768, C=2)          # B*H*W*C = 2^31, one past what the backwards index


def grad_rows(entry, in_grad, par_grad, pair):
    """The gradient contract: both outputs NULL; workspace NULL, one byte short, misaligned; and the order of those checks."""
    n = WORKSPACE[entry]
    return [({in_grad: 0, par_grad: 0}, SHAPE, f"{pair} are both NULL"),
            ({"workspace": 0}, NOMEM, f"workspace needs {n} bytes"),
            ({"workspace_bytes": n - 1}, NOMEM, f"workspace needs {n} bytes"),
            ({"workspace": MISALIGNED}, ALIGN, "workspace must be 8-byte aligned"),
            ({in_grad: 0, par_grad: 0, "workspace": 0}, SHAPE, f"{pair} are both NULL"),
            ({"workspace": MISALIGNED, "workspace_bytes": n - 1}, NOMEM, f"workspace needs {n} bytes")]


def theta_backward(entry, interp):
    shape = "bad shape (theta must be [B,6] or [B,8], B <= 65535)"
    return (nulls("img theta dout", STATE, "NULL buffer") +
            [(dict(B=0), SHAPE, shape), (dict(B=65536), SHAPE, shape), (dict(H=0), SHAPE, shape), (BIG, SHAPE, shape),
             (dict(theta_dim=7), SHAPE, shape), (dict(img=0, B=0), STATE, "NULL buffer")] +
            ([(dict(interp=2), SHAPE, "unknown interp 2"), (dict(interp=-1), SHAPE, "unknown interp -1"),
              (dict(theta_dim=7, interp=2), SHAPE, shape), (dict(interp=2, d_img=0, d_theta=0), SHAPE, "unknown interp 2")] if interp else []) +
            grad_rows(entry, "d_img", "d_theta", "d_img and d_theta"))


def interp_backward():
    shape = "bad shape (B <= 65535)"
    return (nulls("img x y dout", STATE, "NULL buffer") +
            [(dict(B=0), SHAPE, shape), (dict(B=65536), SHAPE, shape), (dict(H=0), SHAPE, shape), (BIG, SHAPE, shape),
             (dict(d_img=0, d_x=0, d_y=0), SHAPE, "d_img, d_x and d_y are all NULL"), (dict(x=0, B=0), STATE, "NULL buffer"),
             (dict(B=0, d_img=0, d_x=0, d_y=0), SHAPE, shape)])


def symmetry_backward(entry, interp):
    shape, pad = "bad shape (B <= 65535)", "the 100-pixel symmetric pad needs H, W >= 100 (got 99x117)"
    return (nulls("img theta dout", STATE, "NULL buffer") +
            [(dict(B=0), SHAPE, shape), (dict(B=65536), SHAPE, shape), (dict(H=0), SHAPE, shape), (BIG, SHAPE, shape),
             (dict(H=99), SHAPE, pad), (dict(W=99), SHAPE, "the 100-pixel symmetric pad needs H, W >= 100 (got 104x99)"),
             (dict(kind=3), SHAPE, "unknown kind 3"), (dict(kind=-1), SHAPE, "unknown kind -1"),
             (dict(theta=0, H=99), STATE, "NULL buffer"), (dict(H=99, kind=3), SHAPE, pad),
             (dict(kind=3, d_img=0, d_theta=0), SHAPE, "unknown kind 3")] +
            ([(dict(interp=2), SHAPE, "unknown interp 2"), (dict(kind=3, interp=2), SHAPE, "unknown kind 3"),
              (dict(interp=2, d_img=0, d_theta=0), SHAPE, "unknown interp 2")] if interp else []) +
            grad_rows(entry, "d_img", "d_theta", "d_img and d_theta"))


def elastic_backward(entry, interp):
    shape = "bad shape (B <= 65535, grid side must be in [2, 16])"
    return (nulls("img theta linv_t dout", STATE, "NULL buffer") +
            [(dict(B=0), SHAPE, shape), (dict(B=65536), SHAPE, shape), (dict(H=0), SHAPE, shape), (BIG, SHAPE, shape),
             (dict(g=1), SHAPE, shape), (dict(g=17), SHAPE, shape), (dict(linv_t=0, g=1), STATE, "NULL buffer"),
             (dict(g=1, d_img=0, d_theta=0), SHAPE, shape)] +
            ([(dict(interp=2), SHAPE, "unknown interp 2"), (dict(g=17, interp=2), SHAPE, shape),
              (dict(interp=2, d_img=0, d_theta=0), SHAPE, "unknown interp 2")] if interp else []) +
            grad_rows(entry, "d_img", "d_theta", "d_img and d_theta"))


def warp_backward(entry, pointers, par_grad):
    shape = "bad shape (B <= 65535, B*Hi*Wi*C < 2^31)"
    return (nulls(pointers, STATE, "NULL buffer") +
            [(dict(B=0), SHAPE, shape), (dict(B=65536), SHAPE, shape), (dict(H=0), SHAPE, shape), (BIG, SHAPE, shape),
             (dict(img=0, B=0), STATE, "NULL buffer"), (dict(dout=0, H=0), STATE, "NULL buffer"),          # pointers, then shape
             ({"B": 0, "d_img": 0, par_grad: 0}, SHAPE, shape)] +
            grad_rows(entry, "d_img", par_grad, "d_img and the matrix gradient"))


ST_THETA = "bad shape (theta must be [B,6] or [B,8])"
ELASTIC = "bad shape (grid side must be in [2, 16])"
COORDS = "bad shape (B <= 65535, grid side must be in [2, 16])"
PAD = "the 100-pixel symmetric pad needs H, W >= 100 (got 99x117)"
ST3D = "bad shape (B <= 65535)"
ST3D_EDGE = "bad shape (edge_size >= 0, B <= 65535)"
VEC = "p must be [B,8] or [B,6], 1 <= warpApprox <= 64"
TPS_G = "grid side %d outside [2, 16] (g = 1 makes L singular)"

TABLE = {
    # ---- forward
    "st_transform": nulls("img theta out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, ST_THETA), (dict(H=0), SHAPE, ST_THETA), (dict(oh=0), SHAPE, ST_THETA), (dict(theta_dim=7), SHAPE, ST_THETA),
        (dict(img=0, B=0), STATE, "NULL buffer")],
    "st_transform_interp": nulls("img theta out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, ST_THETA), (dict(B=65536), SHAPE, ST_THETA), (dict(H=0), SHAPE, ST_THETA), (dict(theta_dim=7), SHAPE, ST_THETA),
        (dict(interp=2), SHAPE, "unknown interp 2"), (dict(interp=-1), SHAPE, "unknown interp -1"),
        (dict(out=0, interp=2), STATE, "NULL buffer"), (dict(B=0, interp=2), SHAPE, ST_THETA)],
    "st_bilinear_interp": nulls("img x y out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, "bad shape"), (dict(H=0), SHAPE, "bad shape"), (dict(y=0, H=0), STATE, "NULL buffer")],
    "st_bicubic_interp": nulls("img x y out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, "bad shape"), (dict(B=65536), SHAPE, "bad shape"), (dict(H=0), SHAPE, "bad shape"),
        (dict(y=0, H=0), STATE, "NULL buffer")],
    "st_meshgrid": [(dict(out=0), STATE, "NULL buffer"), (dict(oh=0), SHAPE, "bad shape"), (dict(ow=1 << 30), SHAPE, "bad shape"),
                    (dict(out=0, oh=0), STATE, "NULL buffer")],
    "st_symmetry_transform": nulls("img theta out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, "bad shape"), (dict(B=65536), SHAPE, "bad shape"), (dict(H=0), SHAPE, "bad shape"),
        (dict(oh=(1 << 20) + 1), SHAPE, "bad shape"), (dict(H=99), SHAPE, PAD),
        (dict(W=99), SHAPE, "the 100-pixel symmetric pad needs H, W >= 100 (got 104x99)"),
        (dict(kind=3), SHAPE, "unknown kind 3"), (dict(kind=-1), SHAPE, "unknown kind -1"), (dict(interp=2), SHAPE, "unknown interp 2"),
        (dict(img=0, H=99), STATE, "NULL buffer"), (dict(B=0, H=99), SHAPE, "bad shape"), (dict(H=99, kind=3), SHAPE, PAD),
        (dict(kind=3, interp=2), SHAPE, "unknown kind 3")],
    "st_symmetry_matrix": nulls("theta out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, "bad shape (1 <= B <= 65535)"), (dict(B=65536), SHAPE, "bad shape (1 <= B <= 65535)"),
        (dict(kind=3), SHAPE, "unknown kind 3"), (dict(out=0, B=0), STATE, "NULL buffer"),
        (dict(B=0, kind=3), SHAPE, "bad shape (1 <= B <= 65535)")],
    "st_symmetry_coords": nulls("theta x_out y_out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, "bad shape (B <= 65535)"), (dict(B=65536), SHAPE, "bad shape (B <= 65535)"),
        (dict(oh=0), SHAPE, "bad shape (B <= 65535)"), (dict(kind=3), SHAPE, "unknown kind 3"),
        (dict(theta=0, kind=3), STATE, "NULL buffer"), (dict(oh=0, kind=3), SHAPE, "bad shape (B <= 65535)")],
    "host_tps_linv": [(dict(linv_t=0), STATE, "linv_t is NULL"), (dict(g=1), SHAPE, TPS_G % 1), (dict(g=17), SHAPE, TPS_G % 17),
                      (dict(cap=27), NOMEM, "need 28 floats"), (dict(g=3, cap=107), NOMEM, "need 108 floats"),
                      (dict(linv_t=0, g=1), STATE, "linv_t is NULL"), (dict(g=17, cap=0), SHAPE, TPS_G % 17)],
    "st_elastic_transform": nulls("img theta linv_t out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, ELASTIC), (dict(B=65536), SHAPE, ELASTIC), (dict(H=0), SHAPE, ELASTIC), (dict(g=1), SHAPE, ELASTIC),
        (dict(g=17), SHAPE, ELASTIC), (dict(interp=2), SHAPE, "unknown interp 2"), (dict(linv_t=0, g=1), STATE, "NULL buffer"),
        (dict(g=1, interp=2), SHAPE, ELASTIC)],
    "st_elastic_coords": nulls("theta linv_t x_out y_out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, COORDS), (dict(B=65536), SHAPE, COORDS), (dict(oh=0), SHAPE, COORDS), (dict(g=1), SHAPE, COORDS),
        (dict(g=17), SHAPE, COORDS), (dict(y_out=0, g=17), STATE, "NULL buffer")],
    "homography_warp": nulls("img M out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, "bad shape"), (dict(H=0), SHAPE, "bad shape"), (dict(ow=0), SHAPE, "bad shape"),
        (dict(M=0, B=0), STATE, "NULL buffer")],
    "transform_image": nulls("img ref pM out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, "bad shape"), (dict(H=0), SHAPE, "bad shape"), (dict(ow=0), SHAPE, "bad shape"),
        (dict(ref=0, B=0), STATE, "NULL buffer")],
    "vec2mtrx": nulls("p out", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, VEC), (dict(dim=7), SHAPE, VEC), (dict(warp_approx=0), SHAPE, VEC), (dict(warp_approx=65), SHAPE, VEC),
        (dict(p=0, dim=7), STATE, "NULL buffer")],
    # ---- backward
    "st_transform_backward": theta_backward("st_transform_backward", False),
    "st_transform_interp_backward": theta_backward("st_transform_interp_backward", True),
    "st_bilinear_interp_backward": interp_backward(),
    "st_bicubic_interp_backward": interp_backward(),
    "st_symmetry_transform_backward": symmetry_backward("st_symmetry_transform_backward", False),
    "st_symmetry_transform_interp_backward": symmetry_backward("st_symmetry_transform_interp_backward", True),
    "st_elastic_transform_backward": elastic_backward("st_elastic_transform_backward", False),
    "st_elastic_transform_interp_backward": elastic_backward("st_elastic_transform_interp_backward", True),
    "homography_warp_backward": warp_backward("homography_warp_backward", "img M dout", "d_M"),
    "transform_image_backward": warp_backward("transform_image_backward", "img ref pM dout", "d_pM"),
    "vec2mtrx_backward": nulls("p d_out d_p", STATE, "NULL buffer") + [
        (dict(B=0), SHAPE, VEC), (dict(dim=7), SHAPE, VEC), (dict(warp_approx=0), SHAPE, VEC), (dict(warp_approx=65), SHAPE, VEC),
        (dict(d_p=0, B=0), STATE, "NULL buffer")],
    # ---- the 3-D volume family: shape, then pointers
    "st3d_meshgrid": [(dict(od=0), SHAPE, "bad shape (at most 2^38 voxels)"), (dict(ow=(1 << 24) + 1), SHAPE, "bad shape (at most 2^38 voxels)"),
                      (dict(out=0), STATE, "NULL buffer"), (dict(out=0, od=0), SHAPE, "bad shape (at most 2^38 voxels)")],
    "st3d_bilinear_interp": [
        (dict(B=0), SHAPE, ST3D_EDGE), (dict(B=65536), SHAPE, ST3D_EDGE), (dict(H=0), SHAPE, ST3D_EDGE), (dict(edge_size=-1), SHAPE, ST3D_EDGE),
        (dict(vol=0, B=0), SHAPE, ST3D_EDGE), (dict(out=0, edge_size=-1), SHAPE, ST3D_EDGE)] + nulls("vol x y z out", STATE, "NULL buffer"),
    "st3d_transform": [
        (dict(B=0), SHAPE, ST3D), (dict(B=65536), SHAPE, ST3D), (dict(H=0), SHAPE, ST3D), (dict(od=0), SHAPE, ST3D),
        (dict(vol=0, B=0), SHAPE, ST3D)] + nulls("vol theta out", STATE, "NULL buffer"),
    "st3d_transform_backward": [
        (dict(B=0), SHAPE, ST3D), (dict(B=65536), SHAPE, ST3D), (dict(H=0), SHAPE, ST3D), (dict(od=0), SHAPE, ST3D),
        (dict(vol=0, B=0), SHAPE, ST3D), (dict(B=0, d_vol=0, d_theta=0), SHAPE, ST3D),
        (dict(dout=0, d_vol=0, d_theta=0), STATE, "NULL buffer")] + nulls("vol theta dout", STATE, "NULL buffer") +
        grad_rows("st3d_transform_backward", "d_vol", "d_theta", "d_vol and d_theta"),
    "st3d_bilinear_interp_backward": [
        (dict(B=0), SHAPE, ST3D_EDGE), (dict(B=65536), SHAPE, ST3D_EDGE), (dict(H=0), SHAPE, ST3D_EDGE), (dict(edge_size=-1), SHAPE, ST3D_EDGE),
        (dict(z=0, edge_size=-1), SHAPE, ST3D_EDGE), (dict(d_vol=0, dx=0, dy=0, dz=0), SHAPE, "d_vol, dx, dy and dz are all NULL"),
        (dict(dout=0, d_vol=0, dx=0, dy=0, dz=0), STATE, "NULL buffer")] + nulls("vol x y z dout", STATE, "NULL buffer"),
}

ROWS = [(entry, bad, code, tail) for entry, rows in TABLE.items() for bad, code, tail in rows]


def test_every_moved_entry_point_has_rows():
    assert set(TABLE) == set(SIGNATURES)
    moved = [n[len("vstab_"):] for n in _lib.EXPORTS
             if n.startswith(("vstab_st_", "vstab_st3d_", "vstab_homography_warp", "vstab_transform_image", "vstab_vec2mtrx", "vstab_host_tps_linv"))
             and not n.endswith("_workspace_bytes")]
    assert sorted(moved) == sorted(TABLE)


@pytest.mark.parametrize("entry,bad,code,tail", ROWS, ids=[f"{e}-{'+'.join(f'{k}={v}' for k, v in b.items())}" for e, b, _, _ in ROWS])
def test_refusal(entry, bad, code, tail):
    assert call(entry, **bad) == (code, f"{entry}: {tail}")


# ---- the size queries: 0 for a shape the backward would refuse, and the value for the well-formed shape of each family
SIZES = {
    "st_transform_backward": ("B H W C oh ow", {}, [dict(B=0), dict(B=65536), dict(H=0), dict(ow=0)]),
    "st_symmetry_transform_backward": ("B H W C oh ow", SYMMETRIC, [dict(B=0), dict(B=65536), dict(H=0), dict(H=99), dict(W=99),
                                                                    dict(oh=(1 << 20) + 1)]),
    "st_elastic_transform_backward": ("B H W C g oh ow", {}, [dict(B=0), dict(B=65536), dict(H=0), dict(g=1), dict(g=17)]),
    "st3d_transform_backward": ("B D H W C od oh ow", VOLUME, [dict(B=0), dict(B=65536), dict(H=0), dict(od=0)]),
    "homography_warp_backward": ("B H W C oh ow", {}, [dict(B=0), dict(B=65536), dict(H=0), dict(ow=0)]),
}


@pytest.mark.parametrize("entry", SIZES)
def test_workspace_bytes(entry):
    names, family, refused = SIZES[entry]
    query = getattr(_lib.lib(), f"vstab_{entry}_workspace_bytes")
    good = {**DEFAULTS, **family}
    assert query(*(good[n] for n in names.split())) == WORKSPACE[entry]
    for bad in refused:
        values = {**good, **bad}
        assert query(*(values[n] for n in names.split())) == 0, bad
