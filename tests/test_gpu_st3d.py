"""The 3-D volume transformer on the GPU (AffineVolumeTransformer, bilinear_interp3d, _meshgrid3d; csrc/sampler3d_ops.hip),
forward: bit-exact (torch.equal) against the fp32 restatement tests/st3d_ref.py.  The output sizes are derived from the brick
the kernels ship with, so that every axis has at least one full and one partial brick."""
import math

import pytest
import torch

from coupe.optical_flow_based_deep_video_stabilization_amd import _lib, spatial_transformer as st
from tests import st3d_ref as ref

pytestmark = pytest.mark.gpu
BZ, BY, BX = ref.brick()
OUT = (BZ + 1, 2 * BY + 3, 2 * BX + 5)
VOL = (5, 7, 9)


def affine3(rx, ry, rz, scale, shift):
    """row-major 3x4: scale * Rz Ry Rx (degrees) and a shift"""
    a, b, c = (math.radians(v) for v in (rx, ry, rz))
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])
    Ry = torch.tensor([[math.cos(b), 0, math.sin(b)], [0, 1, 0], [-math.sin(b), 0, math.cos(b)]])
    Rz = torch.tensor([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    M = torch.cat([scale * (Rz @ Ry @ Rx), torch.tensor(shift).reshape(3, 1)], 1)
    return M.reshape(-1).float()


NEAR_IDENTITY = torch.stack([affine3(12.0, -7.0, 20.0, 1.1, (0.05, -0.1, 0.03)), affine3(-18.0, 15.0, -5.0, 0.9, (-0.08, 0.02, 0.1))])
IDENTITY = torch.tensor([1.0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0])


def _vol(C_, seed, dims=VOL, B=2):
    return torch.rand(B, *dims, C_, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("C_", [1, 2, 3])
def test_transform_near_identity_is_bit_exact(C_):
    vol = _vol(C_, 40 + C_)
    want = ref.transform(vol, NEAR_IDENTITY, OUT)
    assert float((want == 0).float().mean()) < 0.5
    tr = st.AffineVolumeTransformer(OUT)
    got = tr.transform(vol.cuda(), NEAR_IDENTITY.cuda())
    assert got.shape == (2, *OUT, C_) and tr.param_dim == 12
    assert torch.equal(got.cpu(), want)
    assert torch.equal(tr.voxel_grid.cpu(), ref.meshgrid3d(OUT))


def _wild_thetas():
    nan_row = IDENTITY.clone()
    nan_row[4:8] = float("nan")
    inf_row = IDENTITY.clone()
    inf_row[8], inf_row[3] = float("inf"), -float("inf")
    bounds = IDENTITY.clone()
    bounds[0] = 1.25                       # W = 9: x_s = +-1.25 at the grid's ends is v = -1 and v = 9 exactly, the clip bounds
    return {
        "scale3": torch.stack([affine3(30.0, 10.0, -40.0, 3.0, (0.2, -0.3, 0.1)), affine3(0.0, 0.0, 0.0, 3.0, (0.0, 0.0, 0.0))]),
        "nan_and_inf_rows": torch.stack([nan_row, inf_row]),
        "identity_and_clip_bounds": torch.stack([IDENTITY, bounds]),         # the identity lands exactly on -1 and 1
    }


@pytest.mark.parametrize("name", ["scale3", "nan_and_inf_rows", "identity_and_clip_bounds"])
@pytest.mark.parametrize("dims,out", [(VOL, OUT), ((1, 7, 9), OUT), (VOL, (1, OUT[1], OUT[2]))])
def test_transform_wild_maps_are_bit_exact(name, dims, out):
    theta = _wild_thetas()[name]
    vol = _vol(2, 7, dims)
    want = ref.transform(vol, theta, out)
    got = st.AffineVolumeTransformer(out).transform(vol.cuda(), theta.cuda())
    assert torch.isfinite(got).all()
    assert torch.equal(got.cpu(), want)


def special_coords(n, g, lo=-1.6, hi=1.6):
    """random coordinates with the exact landings in front: -1, 1, the clip bounds of W = 9 for edge sizes 0..2, NaN, +-inf"""
    v = torch.rand(n, generator=g) * (hi - lo) + lo
    special = torch.tensor([-1.0, 1.0, -1.25, 1.25, -1.5, 1.5, float("nan"), float("inf"), -float("inf"), 0.0, 1.0 + 1e-7, -3.0, 7.5])
    v[:special.numel()] = special
    return v, special.numel()


@pytest.mark.parametrize("edge", [0, 1, 2])
@pytest.mark.parametrize("C_", [1, 3])
def test_explicit_coordinates_are_bit_exact(edge, C_):
    g = torch.Generator().manual_seed(90 + edge)
    vol = _vol(C_, 50 + edge)
    n = 2 * OUT[0] * OUT[1] * OUT[2]
    x, k = special_coords(n, g)
    y, z = special_coords(n, g)[0].roll(1), special_coords(n, g)[0].roll(2)
    want = ref.bilinear_interp3d(vol, x, y, z, OUT, edge)
    got = st.bilinear_interp3d(vol.cuda(), x.cuda(), y.cuda(), z.cuda(), OUT, edge_size=edge)
    assert got.shape == (n, C_)
    assert torch.equal(got.cpu(), want)
    if edge == 1:
        assert torch.equal(st._interpolate3d(vol.cuda(), x.cuda(), y.cuda(), z.cuda(), OUT, method='anything').cpu(), want)
        assert torch.equal(st.bilinear_interp3d(vol.cuda(), x.cuda(), y.cuda(), z.cuda(), OUT).cpu(), want)        # edge_size defaults to 1


@pytest.mark.parametrize("out", [OUT, (1, 1, 1), (1, 5, 2), (4, 1, 300)])
def test_meshgrid3d_is_bit_exact(out):
    got = st._meshgrid3d(out)
    assert got.shape == (4 * out[0] * out[1] * out[2],)
    assert torch.equal(got.cpu(), ref.meshgrid3d(out))


def test_argument_errors():
    vol, theta = _vol(1, 1).cuda(), NEAR_IDENTITY.cuda()
    tr = st.AffineVolumeTransformer(OUT)
    n = 2 * OUT[0] * OUT[1] * OUT[2]
    c = torch.zeros(n, device="cuda")
    with pytest.raises(ValueError):
        tr.transform(vol.cpu(), theta)                                   # a CPU tensor
    with pytest.raises(ValueError):
        tr.transform(vol[:, 0], theta)                                   # wrong rank
    with pytest.raises(ValueError):
        tr.transform(vol, theta[:, :11])                                 # theta not [B,12]
    with pytest.raises(ValueError):
        st.bilinear_interp3d(vol, c, c, c, OUT, edge_size=-1)
    with pytest.raises(ValueError):
        st.bilinear_interp3d(vol.cpu(), c, c, c, OUT)
    with pytest.raises(ValueError):
        st.bilinear_interp3d(vol, c[:-1], c, c, OUT)
    with pytest.raises(ValueError):
        st.AffineVolumeTransformer((4, 4))
    # an oversized shape is refused by the C entry points before any pointer is looked at or anything is launched
    L = _lib.lib()
    E_SHAPE, big = -1, 1 << 15
    assert L.vstab_st3d_transform(None, 1, 8, 8, 8, 1, None, None, big, big, big, None) == E_SHAPE                  # 2^37 bricks
    assert L.vstab_st3d_transform(None, 1, 8, 8, 8, 1, None, None, 1 << 25, 1, 1, None) == E_SHAPE                  # an extent over 2^24
    assert L.vstab_st3d_transform(None, 1, 1 << 14, 1 << 14, 1 << 14, 1, None, None, 4, 4, 4, None) == E_SHAPE      # 2^42 voxels to read
    assert L.vstab_st3d_bilinear_interp(None, 1, 8, 8, 8, 1, None, None, None, big, big, big, 1, None, None) == E_SHAPE
    assert L.vstab_st3d_bilinear_interp(None, 1, 8, 8, 8, 1, None, None, None, 4, 4, 4, -1, None, None) == E_SHAPE
    assert L.vstab_st3d_meshgrid(None, big, big, big, None) == E_SHAPE
    assert L.vstab_st3d_transform_backward_workspace_bytes(1, 8, 8, 8, 1, big, big, big) == 0
    assert L.vstab_st3d_transform_backward(None, 1, 8, 8, 8, 1, None, None, big, big, big, None, 0, None, None, 0, None) == E_SHAPE
    assert L.vstab_st3d_bilinear_interp_backward(None, 65536, 8, 8, 8, 1, None, None, None, 4, 4, 4, 1, None, None, 0, None, None, None, None) == E_SHAPE
    assert L.vstab_st3d_transform(None, 1, 8, 8, 8, 1, None, None, 4, 4, 4, None) == -6                             # VSTAB_E_STATE: NULL buffers
