// C ABI of the image-similarity measures of utils.py (tf_ssim :91-124, tf_ms_ssim :126-166): argument checks, the 1-D window and
// the workspace sizes.  The kernels are in ssim_ops.hip.
#include <cmath>

#include "api_internal.h"

using namespace vstab;

namespace {

// _tf_fspecial_gauss (utils.py:74-89) is g[i,j] = e_i e_j / sum(e_i e_j) with e_k = exp(-c_k^2 / (2 sigma^2)) and c_k running over
// -size//2+1 .. size//2 (floor division: -3..4 for size 8), i.e. the outer product of e / sum(e) with itself.
bool ssim_window(int size, float sigma, SsimWindow &win)
{
    if (size < 1 || size > SSIM_MAX_SIZE || !(sigma > 0.f) || !std::isfinite(sigma)) return false;
    const int first = -((size + 1) / 2) + 1;           // Python's -size//2 + 1
    double e[SSIM_MAX_SIZE], sum = 0.0;
    for (int k = 0; k < size; ++k) {
        const double c = (double)(first + k);
        e[k] = std::exp(-(c * c) / (2.0 * (double)sigma * (double)sigma));
        sum += e[k];
    }
    if (!(sum > 0.0)) return false;
    for (int k = 0; k < SSIM_MAX_SIZE; ++k) win.w[k] = k < size ? (float)(e[k] / sum) : 0.f;
    return true;
}

// B >= 1, size 1..11, H, W >= size, every tensor below 2^31 elements, grid dimensions within 65535
bool ssim_shape_ok(int B, int H, int W, int size)
{
    if (B < 1 || B > 65535 || size < 1 || size > SSIM_MAX_SIZE || H < size || W < size) return false;
    if ((long long)B * H * W >= (1LL << 31)) return false;
    return (H + 15) / 16 <= 65535;
}

bool pool_shape_ok(int B, int H, int W, int C)
{
    return B >= 1 && H >= 1 && W >= 1 && C >= 1 && (long long)B * H * W * C < (1LL << 31);
}

}  // namespace

extern "C" size_t vstab_ssim_forward_workspace_bytes(int B, int H, int W, int size)
{
    if (!ssim_shape_ok(B, H, W, size)) return 0;
    return a256((size_t)B * ssim_tiles_per_sample(H - size + 1, W - size + 1) * sizeof(float));
}

extern "C" int vstab_ssim_forward(const float *img1, const float *img2, int B, int H, int W, int size, float sigma, float *map, float *means,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (!img1 || !img2 || (!map && !means) || (means && !workspace)) return fail(nullptr, VSTAB_E_STATE, "ssim_forward: NULL buffer");
    SsimWindow win;
    if (!ssim_shape_ok(B, H, W, size) || !ssim_window(size, sigma, win))
        return fail(nullptr, VSTAB_E_SHAPE, "ssim_forward: need B >= 1, 1 <= size <= %d, H, W >= size, sigma > 0 and fewer than 2^31 elements",
                    SSIM_MAX_SIZE);
    if (means) {
        if (((uintptr_t)workspace) & 3) return fail(nullptr, VSTAB_E_ALIGN, "ssim_forward: workspace must be 4-byte aligned");
        const size_t need = vstab_ssim_forward_workspace_bytes(B, H, W, size);
        if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "ssim_forward: workspace %zu < %zu bytes", workspace_bytes, need);
    }
    HIP_TRY(nullptr, launch_ssim_forward(img1, img2, B, H, W, size, win, map, means, (float *)workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_ssim_backward_workspace_bytes(int B, int H, int W, int size)
{
    if (!ssim_shape_ok(B, H, W, size)) return 0;
    return a256((size_t)5 * B * (H - size + 1) * (W - size + 1) * sizeof(float));
}

extern "C" int vstab_ssim_backward(const float *img1, const float *img2, int B, int H, int W, int size, float sigma, const float *dmap,
                                   const float *dmeans, float *d_img1, float *d_img2, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!img1 || !img2 || (!dmap && !dmeans) || !workspace) return fail(nullptr, VSTAB_E_STATE, "ssim_backward: NULL buffer");
    SsimWindow win;
    if (!ssim_shape_ok(B, H, W, size) || !ssim_window(size, sigma, win))
        return fail(nullptr, VSTAB_E_SHAPE, "ssim_backward: need B >= 1, 1 <= size <= %d, H, W >= size, sigma > 0 and fewer than 2^31 elements",
                    SSIM_MAX_SIZE);
    if (!d_img1 && !d_img2) return fail(nullptr, VSTAB_E_SHAPE, "ssim_backward: no gradient asked for");
    if (((uintptr_t)workspace) & 3) return fail(nullptr, VSTAB_E_ALIGN, "ssim_backward: workspace must be 4-byte aligned");
    const size_t need = vstab_ssim_backward_workspace_bytes(B, H, W, size);
    if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "ssim_backward: workspace %zu < %zu bytes", workspace_bytes, need);
    HIP_TRY(nullptr, launch_ssim_backward(img1, img2, B, H, W, size, win, dmap, dmeans, d_img1, d_img2, (float *)workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_avgpool2x2_same(const float *x, int B, int H, int W, int C, float *out, void *stream)
{
    if (!x || !out) return fail(nullptr, VSTAB_E_STATE, "avgpool2x2_same: NULL buffer");
    if (!pool_shape_ok(B, H, W, C)) return fail(nullptr, VSTAB_E_SHAPE, "avgpool2x2_same: bad shape");
    HIP_TRY(nullptr, launch_avgpool2x2_same(x, B, H, W, C, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_avgpool2x2_same_backward(const float *dout, int B, int H, int W, int C, float *dx, void *stream)
{
    if (!dout || !dx) return fail(nullptr, VSTAB_E_STATE, "avgpool2x2_same_backward: NULL buffer");
    if (!pool_shape_ok(B, H, W, C)) return fail(nullptr, VSTAB_E_SHAPE, "avgpool2x2_same_backward: bad shape");
    HIP_TRY(nullptr, launch_avgpool2x2_same_backward(dout, B, H, W, C, dx, (hipStream_t)stream));
    return VSTAB_OK;
}
