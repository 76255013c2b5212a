// C ABI of NLDF's objective (NLDF.py:79-100, :136-171): argument checks and workspace sizes.  The kernels are in nldf_loss_ops.hip.
#include "api_internal.h"

using namespace vstab;

namespace {

bool image_shape_ok(int B, int H, int W, int C, int cmax)
{
    return B >= 1 && H >= 1 && W >= 1 && C >= 1 && C <= cmax && (long long)B * H * W * C < (1LL << 31);
}

}  // namespace

extern "C" int vstab_sobel_magnitude(const float *x, int B, int H, int W, int C, float *out, void *stream)
{
    if (!x || !out) return fail(nullptr, VSTAB_E_STATE, "sobel_magnitude: NULL buffer");
    if (!image_shape_ok(B, H, W, C, 4))
        return fail(nullptr, VSTAB_E_SHAPE, "sobel_magnitude: need B, H, W >= 1, 1 <= C <= 4 and fewer than 2^31 elements");
    HIP_TRY(nullptr, launch_sobel_magnitude(x, B, H, W, C, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_sobel_magnitude_backward(const float *x, const float *dout, int B, int H, int W, int C, float *dx, void *stream)
{
    if (!x || !dout || !dx) return fail(nullptr, VSTAB_E_STATE, "sobel_magnitude_backward: NULL buffer");
    if (!image_shape_ok(B, H, W, C, 4))
        return fail(nullptr, VSTAB_E_SHAPE, "sobel_magnitude_backward: need B, H, W >= 1, 1 <= C <= 4 and fewer than 2^31 elements");
    HIP_TRY(nullptr, launch_sobel_magnitude_backward(x, dout, B, H, W, C, dx, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_nldf_loss_workspace_bytes(int B, int H, int W)
{
    if (!image_shape_ok(B, H, W, 2, 2)) return 0;
    return a256((2 + 5 * nldf_loss_tiles(B, H, W)) * sizeof(double));
}

extern "C" int vstab_nldf_loss(const float *score, const float *label, int B, int H, int W, float contour_th, float *scalars4, float *prob_grad,
                               float *label_grad, float *dscore, float dscale, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!score || !label || !scalars4 || !workspace) return fail(nullptr, VSTAB_E_STATE, "nldf_loss: NULL buffer");
    if (!image_shape_ok(B, H, W, 2, 2)) return fail(nullptr, VSTAB_E_SHAPE, "nldf_loss: need B, H, W >= 1 and fewer than 2^31 elements");
    if ((((uintptr_t)score) | ((uintptr_t)label) | ((uintptr_t)dscore) | ((uintptr_t)workspace)) & 7)
        return fail(nullptr, VSTAB_E_ALIGN, "nldf_loss: score, label, dscore and the workspace must be 8-byte aligned");
    const size_t need = vstab_nldf_loss_workspace_bytes(B, H, W);
    if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "nldf_loss: workspace %zu < %zu bytes", workspace_bytes, need);
    HIP_TRY(nullptr, launch_nldf_loss(score, label, B, H, W, contour_th, scalars4, prob_grad, label_grad, dscore, dscale, (double *)workspace,
                                      (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_nldf_reduce_workspace_bytes(long long n)
{
    if (n < 1 || n >= (1LL << 31)) return 0;
    return a256((2 + 3 * (size_t)nldf_reduce_blocks(n)) * sizeof(double));
}

extern "C" int vstab_nldf_reduce(int mode, const float *a, const float *b, long long n, float wd, float *value, float *grad, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    if (!a || (!b && mode != VSTAB_NLDF_REDUCE_L2) || !value || !workspace) return fail(nullptr, VSTAB_E_STATE, "nldf_reduce: NULL buffer");
    if (mode < VSTAB_NLDF_REDUCE_IOU || mode > VSTAB_NLDF_REDUCE_L2 || n < 1 || n >= (1LL << 31))
        return fail(nullptr, VSTAB_E_SHAPE, "nldf_reduce: need mode 0..2 and 1 <= n < 2^31");
    if (((uintptr_t)workspace) & 7) return fail(nullptr, VSTAB_E_ALIGN, "nldf_reduce: the workspace must be 8-byte aligned");
    const size_t need = vstab_nldf_reduce_workspace_bytes(n);
    if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "nldf_reduce: workspace %zu < %zu bytes", workspace_bytes, need);
    HIP_TRY(nullptr, launch_nldf_reduce(mode, a, b, n, wd, value, grad, (double *)workspace, (hipStream_t)stream));
    return VSTAB_OK;
}
