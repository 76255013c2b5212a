"""NumPy restatement of the flow colour code that flow_vis.py promises (the Middlebury code of the reference's flow_to_image), with
the dtype of every step written out so that the result does not depend on the installed NumPy's casting rules: float32 up to the
wheel lookup, float64 from there.

  unknown = |u| > 1e7 or |v| > 1e7        -> counts as (0,0) in the maximum, black in img
  nan     = u or v is NaN                 -> left out of the maximum, black in img
  maxrad  = sqrt(max(u*u + v*v)) in float32 over the pixels that count (0 when none does)
  d = maxrad > 0 ? maxrad : 2^-52;  un = u / d, vn = v / d                     (float32; unknown and NaN pixels are +0 here)
  rad = sqrt(un*un + vn*vn);  ang = arctan2(-vn, -un);  a = ang / float32(pi)  (float32)
  fk = (a + 1) / 2 * 54 + 1;  k0 = floor(fk);  k1 = k0 + 1, 56 -> 1;  f = fk - k0   (float32; the subtraction is exact)
  col = (1 - f) * wheel[k0-1] / 255 + f * wheel[k1-1] / 255                    (float64)
  col = rad <= 1 ? 1 - rad * (1 - col) : 0.75 * col;  img = uint8(floor(255 * col))
  anglemap = uint8(trunc(a * 127 + 128)) in float32, in three channels; unknown and NaN pixels give 1, the value of (+0, +0)

angle_ulps = k moves `ang`, the float32 result of arctan2, by k units in its last place before anything else is done with it (the
one step whose rounding differs between math libraries), held within [-float32(pi), float32(pi)], the range an atan2f returns."""
import numpy as np

F32 = np.float32
SEGMENTS = (15, 6, 4, 11, 13, 6)            # RY, YG, GC, CB, BM, MR
NCOLS = sum(SEGMENTS)
UNKNOWN = F32(1e7)
PI32 = F32(np.pi)
EPS = F32(2.0 ** -52)


def color_wheel():
    """[55,3] float64.  Red -> yellow -> green -> cyan -> blue -> magenta -> red, written out segment by segment."""
    up = lambda n: np.floor(255.0 * np.arange(n, dtype=np.float64) / n)          # noqa: E731
    ry, yg, gc, cb, bm, mr = SEGMENTS
    rows = []
    rows += [(255.0, g, 0.0) for g in up(ry)]
    rows += [(255.0 - r, 255.0, 0.0) for r in up(yg)]
    rows += [(0.0, 255.0, b) for b in up(gc)]
    rows += [(0.0, 255.0 - g, 255.0) for g in up(cb)]
    rows += [(r, 0.0, 255.0) for r in up(bm)]
    rows += [(255.0, 0.0, 255.0 - b) for b in up(mr)]
    return np.array(rows, dtype=np.float64)


def shift_ulps(x, k):
    """float32 array x moved by k units in the last place (through zero correctly: -0 and +0 are one step apart in this order)"""
    x = np.asarray(x, dtype=F32)
    if k == 0:
        return x
    i = x.view(np.int32).astype(np.int64)
    key = np.where(i < 0, -(i & 0x7FFFFFFF) - 1, i)                  # monotone in the float's value: -0 -> -1, +0 -> 0
    key = key + k
    i = np.where(key < 0, (-(key + 1)) | 0x80000000, key)
    return i.astype(np.uint32).view(F32)


def max_radius(flow):
    """float32 [B] for flow [B,H,W,2]"""
    flow = np.asarray(flow, dtype=F32)
    u, v = flow[..., 0], flow[..., 1]
    unknown = (np.abs(u) > UNKNOWN) | (np.abs(v) > UNKNOWN)
    nan = np.isnan(u) | np.isnan(v)
    with np.errstate(invalid="ignore", over="ignore"):
        s = (u * u + v * v).astype(F32)
    s = np.where(unknown | nan, F32(0), s).astype(F32)
    return np.sqrt(s.reshape(s.shape[0], -1).max(axis=1)).astype(F32)


def flow_to_image(flow, maxrad=None, angle_ulps=0):
    """flow [B,H,W,2] -> (img [B,H,W,3] uint8, anglemap [B,H,W,3] uint8, maxrad [B] float32).  maxrad: None or [B]."""
    flow = np.array(flow, dtype=F32)                                    # a copy: the caller's array stays as it is
    assert flow.ndim == 4 and flow.shape[3] == 2
    B = flow.shape[0]
    maxrad = max_radius(flow) if maxrad is None else np.broadcast_to(np.asarray(maxrad, dtype=F32).reshape(-1), (B,)).copy()
    u, v = flow[..., 0], flow[..., 1]
    dead = (np.abs(u) > UNKNOWN) | (np.abs(v) > UNKNOWN) | np.isnan(u) | np.isnan(v)
    u = np.where(dead, F32(0), u).astype(F32)
    v = np.where(dead, F32(0), v).astype(F32)
    d = np.where(maxrad > 0, maxrad, EPS).astype(F32).reshape(B, 1, 1)
    with np.errstate(over="ignore", invalid="ignore"):
        un = (u / d).astype(F32)
        vn = (v / d).astype(F32)
        rad = np.sqrt((un * un + vn * vn).astype(F32)).astype(F32)
    ang = np.arctan2(-vn, -un).astype(F32)
    ang = np.clip(shift_ulps(ang, angle_ulps), -PI32, PI32).astype(F32)
    a = (ang / PI32).astype(F32)
    fk = ((a + F32(1)) / F32(2) * F32(NCOLS - 1) + F32(1)).astype(F32)
    k0f = np.floor(fk).astype(F32)
    k0 = k0f.astype(np.int64)
    assert k0.min() >= 1 and k0.max() <= NCOLS
    k1 = np.where(k0 == NCOLS, 1, k0 + 1)
    f = (fk - k0f).astype(F32).astype(np.float64)
    wheel = color_wheel()
    rad64 = rad.astype(np.float64)
    img = np.zeros(flow.shape[:3] + (3,), dtype=np.uint8)
    for c in range(3):
        col0 = wheel[k0 - 1, c] / 255.0
        col1 = wheel[k1 - 1, c] / 255.0
        col = (1.0 - f) * col0 + f * col1
        with np.errstate(invalid="ignore"):
            col = np.where(rad <= F32(1), 1.0 - rad64 * (1.0 - col), 0.75 * col)
        img[..., c] = np.where(dead, 0.0, np.floor(255.0 * col)).astype(np.uint8)
    gray = np.trunc((a * F32(127) + F32(128)).astype(F32)).astype(np.uint8)
    return img, np.repeat(gray[..., None], 3, axis=3), maxrad


def interval(flow, maxrad=None, k=0):
    """per byte the smallest and largest value over angle_ulps in -k..k: (img_lo, img_hi, ang_lo, ang_hi, maxrad)"""
    outs = [flow_to_image(flow, maxrad, s) for s in range(-k, k + 1)]
    imgs, angs = np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
    return imgs.min(0), imgs.max(0), angs.min(0), angs.max(0), outs[0][2]


def radius_above_one(seed=0, tries=200000):
    """A pixel (u, v) whose normalised radius exceeds 1 by rounding alone: with m = sqrt(u*u + v*v), the image's own maximum,
    sqrt((u/m)^2 + (v/m)^2) > 1 in float32.  A seeded search; returns float32 (u, v) of the first hit."""
    rng = np.random.default_rng(seed)
    uv = rng.standard_normal((tries, 2)).astype(F32) * F32(3)
    u, v = uv[:, 0], uv[:, 1]
    m = np.sqrt((u * u + v * v).astype(F32)).astype(F32)
    un, vn = (u / m).astype(F32), (v / m).astype(F32)
    r = np.sqrt((un * un + vn * vn).astype(F32)).astype(F32)
    hit = np.flatnonzero(r > F32(1))
    assert hit.size, "no pixel with a rounded radius above 1 found"
    return u[hit[0]], v[hit[0]]
