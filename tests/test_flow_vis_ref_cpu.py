"""The NumPy restatement of the flow colour code (tests/flow_vis_ref.py) pinned by known answers: the wheel's rows, the colours at the
seam, at zero, at unknown and NaN pixels, and a pixel whose normalised radius exceeds 1 by rounding.  Also: the package's
make_color_wheel agrees with it, and the new symbols are declared, bound and built."""
import os
import re

import numpy as np

from tests import flow_vis_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "coupe", "optical_flow_based_deep_video_stabilization_amd")
NEW_SYMBOLS = ("vstab_flow_to_image_workspace_bytes", "vstab_flow_to_image")
F32 = np.float32


def _image(pixels):
    """1 x n image from a list of (u, v)"""
    return np.array(pixels, dtype=F32).reshape(1, 1, len(pixels), 2)


def test_wheel_rows():
    w = ref.color_wheel()
    assert w.shape == (55, 3) and w.dtype == np.float64
    assert tuple(w[0]) == (255, 0, 0)
    assert tuple(w[15]) == (255, 255, 0)
    assert tuple(w[54]) == (255, 0, 43)
    assert np.array_equal(w, np.floor(w)) and w.min() == 0 and w.max() == 255
    # every row has one channel at 255 and one at 0, the third being the ramp that passes between them
    for row in w:
        assert (row == 255).sum() >= 1 and (row == 0).sum() >= 1
    # the corners of the hue circle: yellow, green, cyan, blue, magenta start the segments
    starts = np.cumsum((0,) + ref.SEGMENTS[:-1])
    assert [tuple(w[s]) for s in starts] == [(255, 0, 0), (255, 255, 0), (0, 255, 0), (0, 255, 255), (0, 0, 255), (255, 0, 255)]
    # neighbouring rows differ in one channel only, and so do the last and the first
    for i in range(55):
        assert ((w[i] != w[(i + 1) % 55]).sum()) == 1


def test_package_wheel_is_the_same():
    from coupe.optical_flow_based_deep_video_stabilization_amd import flow_vis
    w = flow_vis.make_color_wheel()
    assert w.dtype == np.float64 and w.shape == (55, 3)
    assert np.array_equal(w, ref.color_wheel())


def test_seam_zero_and_unknown():
    flow = _image([(1.0, 0.0), (1.0, -0.0), (0.0, 0.0), (2e7, 0.0)])
    keep = flow.copy()
    img, ang, maxrad = ref.flow_to_image(flow)
    assert flow.tobytes() == keep.tobytes()                              # the unknown pixel is still 2e7 in the caller's array
    assert maxrad.dtype == F32 and maxrad[0] == F32(1)                   # the unknown pixel counted as (0,0)
    assert img.dtype == np.uint8 and img.shape == (1, 1, 4, 3)
    assert tuple(img[0, 0, 0]) == (255, 0, 0)
    assert tuple(img[0, 0, 1]) == (255, 0, 43)                           # the sign of zero puts this pixel on the seam's other side
    assert tuple(img[0, 0, 2]) == (255, 255, 255)
    assert tuple(img[0, 0, 3]) == (0, 0, 0)
    # angle map: atan2(-0, -1) = -pi -> 1; atan2(+0, -1) = +pi -> 255; the zero and the unknown pixel are atan2(-0, -0) = -pi -> 1
    assert ang.shape == (1, 1, 4, 3) and [int(x) for x in ang[0, 0, :, 0]] == [1, 255, 1, 1]
    assert np.array_equal(ang[..., 0], ang[..., 1]) and np.array_equal(ang[..., 0], ang[..., 2])


def test_nan_pixel_is_black_and_changes_nothing_else():
    rng = np.random.default_rng(5)
    flow = rng.standard_normal((1, 6, 7, 2)).astype(F32) * F32(4)
    img0, ang0, m0 = ref.flow_to_image(flow)
    for comp in (0, 1):
        bad = flow.copy()
        # not the pixel that holds the maximum: leaving that one out would change the normalisation, as it should
        far = int(np.argmax((flow[0] ** 2).sum(-1)))
        y, x = divmod((far + 1) % 42, 7)
        bad[0, y, x, comp] = np.nan
        img, ang, m = ref.flow_to_image(bad)
        assert m[0] == m0[0]
        assert tuple(img[0, y, x]) == (0, 0, 0) and int(ang[0, y, x, 0]) == 1
        mask = np.ones((6, 7), bool)
        mask[y, x] = False
        assert np.array_equal(img[0][mask], img0[0][mask]) and np.array_equal(ang[0][mask], ang0[0][mask])
    # a sample of nothing but NaN: radius 0, all black
    img, _, m = ref.flow_to_image(np.full((1, 2, 3, 2), np.nan, F32))
    assert m[0] == 0 and not img.any()


def test_all_zero_flow_is_white():
    img, ang, m = ref.flow_to_image(np.zeros((2, 3, 5, 2), F32))
    assert (m == 0).all() and (img == 255).all() and (ang == 1).all()


def test_given_radius_is_used_as_it_is():
    flow = _image([(1.0, 0.0), (0.0, 2.0), (-4.0, 0.0)])
    img, _, m = ref.flow_to_image(flow, maxrad=np.array([8.0], F32))
    assert m[0] == F32(8)
    own, _, m_own = ref.flow_to_image(flow)
    assert m_own[0] == F32(4) and not np.array_equal(img, own)
    # rad = 1/8: col = 1 - (1 - wheel/255) / 8 -> floor(255 * (1 - 1/8)) = 223 in the channels where row 0 is 0
    assert tuple(img[0, 0, 0]) == (255, 223, 223)
    # a radius above 1 (the given maximum is too small) takes the x0.75 branch: (255, 0, 0) -> 191
    img, _, _ = ref.flow_to_image(flow, maxrad=np.array([0.5], F32))
    assert tuple(img[0, 0, 0]) == (191, 0, 0)


def test_radius_above_one_by_rounding():
    u, v = ref.radius_above_one()
    assert u.dtype == F32 and v.dtype == F32
    m = np.sqrt(F32(u * u + v * v)).astype(F32)
    un, vn = F32(u / m), F32(v / m)
    assert np.sqrt(F32(un * un + vn * vn)).astype(F32) > F32(1)
    # alone in its image the pixel is the maximum, its radius rounds above 1, and the colour is the wheel's times 0.75: no channel
    # can exceed floor(255 * 0.75) = 191, whereas the rad <= 1 branch at a radius of 1 gives the wheel's own colour with a 255 in it
    flow = _image([(u, v), (0.0, 0.0)])
    img, _, maxrad = ref.flow_to_image(flow)
    assert maxrad[0] == m
    assert int(img[0, 0, 0].max()) == 191
    assert tuple(img[0, 0, 1]) == (255, 255, 255)
    # one ulp more radius to divide by brings it back under 1 and into the other branch
    img, _, _ = ref.flow_to_image(flow, maxrad=np.array([np.nextafter(m, F32(np.inf))], F32))
    assert int(img[0, 0, 0].max()) >= 254


def test_shift_ulps_and_interval():
    x = np.array([1.0, -1.0, 0.0, -0.0, 3.0], F32)
    assert np.array_equal(ref.shift_ulps(x, 1)[:2], np.array([np.nextafter(F32(1), F32(2)), np.nextafter(F32(-1), F32(0))], F32))
    assert np.array_equal(ref.shift_ulps(ref.shift_ulps(x, 3), -3).view(np.uint32), x.view(np.uint32))
    assert ref.shift_ulps(x, -1)[2].view(np.uint32) == np.uint32(0x80000000)            # +0 - 1 ulp = -0
    assert (np.diff(ref.shift_ulps(np.array([-2.0, -0.0, 0.0, 2.0], F32), 5)) > 0).all()
    flow = np.random.default_rng(1).standard_normal((1, 8, 9, 2)).astype(F32)
    lo, hi, alo, ahi, m = ref.interval(flow, None, 4)
    img, ang, m0 = ref.flow_to_image(flow)
    assert (lo <= img).all() and (img <= hi).all() and (alo <= ang).all() and (ang <= ahi).all() and m[0] == m0[0]
    # the seam pixel's interval reaches both sides; the shifted angle never leaves [-pi, pi]
    lo, hi, _, _, _ = ref.interval(_image([(1.0, 0.0)]), None, 1)
    assert tuple(lo[0, 0, 0]) == (255, 0, 0) and tuple(hi[0, 0, 0]) == (255, 0, 0)


def test_symbols_declared_bound_and_built():
    from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "vstab.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"VSTAB_API\s+\w+\s+" + name + r"\(", header), name
        assert name in _lib.EXPORTS
    assert "flow_vis_ops.hip" in build.SOURCES and "flow_vis_api.cpp" in build.SOURCES
    for s in ("flow_vis_ops.hip", "flow_vis_api.cpp"):
        assert os.path.exists(os.path.join(PKG, "csrc", s))
