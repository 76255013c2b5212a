// C ABI of the theta regressors' blocks (csrc/theta_ops.hip): SYMMETRIC pad, BatchNorm + lrelu(slope) alone and with the 2x2 pool, the
// dense layers.  Every check is made before the first launch, in the order NULL buffer, shape, alignment, workspace.
#include <cstdint>

#include "../../../include/vstab.h"
#include "api_internal.h"
#include "theta_ops.h"
#include "vstab_internal.h"

using namespace vstab;

namespace {
bool misaligned(const void *p, uintptr_t bytes)
{
    return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0;
}

constexpr long long INT31 = 1LL << 31;

bool dense_shape_ok(int B, int K, int N)
{
    return B >= 1 && B <= 32 && K >= 4 && (K & 3) == 0 && N >= 1 && (long long)K * N < (1LL << 40);
}
}  // namespace

extern "C" int vstab_pad_symmetric(const float *x, int B, int H, int W, int C, int p, float *y, int cs_y, void *stream)
{
    if (!x || !y) return fail(nullptr, VSTAB_E_STATE, "pad_symmetric: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || p < 0 || p > H || p > W || cs_y < C || (cs_y & 3) ||
        (long long)B * (H + 2LL * p) * (W + 2LL * p) * cs_y >= INT31)
        return fail(nullptr, VSTAB_E_SHAPE, "pad_symmetric: bad shape (0 <= p <= min(H, W), cs_y >= C and a multiple of 4, y below 2^31 floats)");
    if (misaligned(x, 4) || misaligned(y, 16)) return fail(nullptr, VSTAB_E_ALIGN, "pad_symmetric: x 4-byte, y 16-byte aligned");
    HIP_TRY(nullptr, launch_pad_symmetric(x, B, H, W, C, p, y, cs_y, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_bn_lrelu_slope_inference(float *zy, long long rows, int cs, int c_off, int C, const float *beta, const float *moving_mean,
                                              const float *moving_var, float eps, float slope, int twice, void *stream)
{
    if (!zy || !beta || !moving_mean || !moving_var) return fail(nullptr, VSTAB_E_STATE, "bn_lrelu_slope_inference: NULL buffer");
    if (rows < 1 || C < 1 || c_off < 0 || c_off + C > cs) return fail(nullptr, VSTAB_E_SHAPE, "bn_lrelu_slope_inference: bad shape");
    if ((C & 3) || (cs & 3) || (c_off & 3) || misaligned(zy, 16) || misaligned(beta, 16) || misaligned(moving_mean, 16) ||
        misaligned(moving_var, 16))
        return fail(nullptr, VSTAB_E_ALIGN, "bn_lrelu_slope_inference: channels multiples of 4, 16-byte aligned buffers");
    HIP_TRY(nullptr, launch_bn_lrelu_slope_inference(zy, rows, cs, c_off, C, beta, moving_mean, moving_var, eps, slope, twice ? 1 : 0,
                                                     (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_bn_lrelu_slope_pool_inference(const float *z, int B, int H, int W, int C, const float *beta, const float *moving_mean,
                                                   const float *moving_var, float eps, float slope, int twice, float *out, void *stream)
{
    if (!z || !beta || !moving_mean || !moving_var || !out) return fail(nullptr, VSTAB_E_STATE, "bn_lrelu_slope_pool_inference: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || (long long)B * H * W * C >= INT31)
        return fail(nullptr, VSTAB_E_SHAPE, "bn_lrelu_slope_pool_inference: bad shape (B*H*W*C < 2^31)");
    if ((C & 3) || misaligned(z, 16) || misaligned(out, 16) || misaligned(beta, 16) || misaligned(moving_mean, 16) || misaligned(moving_var, 16))
        return fail(nullptr, VSTAB_E_ALIGN, "bn_lrelu_slope_pool_inference: channels a multiple of 4, 16-byte aligned buffers");
    HIP_TRY(nullptr, launch_bn_lrelu_slope_pool_inference(z, B, H, W, C, beta, moving_mean, moving_var, eps, slope, twice ? 1 : 0, out,
                                                          (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_host_dense_plan(int K, int N, int32_t *slab_rows, int32_t *slabs)
{
    if (!slab_rows || !slabs) return fail(nullptr, VSTAB_E_STATE, "dense_plan: NULL buffer");
    *slab_rows = *slabs = 0;
    if (!dense_shape_ok(1, K, N)) return fail(nullptr, VSTAB_E_SHAPE, "dense_plan: bad shape (K a multiple of 4, N >= 1, K*N < 2^40)");
    const DensePlan d = dense_plan(K, N);
    *slab_rows = d.rows;
    *slabs = d.slabs;
    return VSTAB_OK;
}

extern "C" size_t vstab_dense_forward_workspace_bytes(int B, int K, int N)
{
    if (!dense_shape_ok(B, K, N)) return 0;
    return (size_t)dense_plan(K, N).slabs * B * N * sizeof(float);
}

extern "C" int vstab_dense_forward(const float *x, int B, int K, int N, const float *W, const float *b, int act, float slope, const float *scale,
                                   const float *shift, float *y, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !W || !b || !y || (act == VSTAB_DENSE_TANH_AFFINE && (!scale || !shift)))
        return fail(nullptr, VSTAB_E_STATE, "dense_forward: NULL buffer");
    if (!dense_shape_ok(B, K, N) || act < VSTAB_DENSE_IDENTITY || act > VSTAB_DENSE_TANH_AFFINE)
        return fail(nullptr, VSTAB_E_SHAPE, "dense_forward: bad shape (1 <= B <= 32, K a multiple of 4, N >= 1, K*N < 2^40, act in 0..3)");
    if (misaligned(x, 16) || misaligned(y, 16) || misaligned(W, (N & 3) ? 4 : 16) || misaligned(b, 4))
        return fail(nullptr, VSTAB_E_ALIGN, "dense_forward: x, y (and W when N %% 4 == 0) 16-byte aligned");
    const size_t need = vstab_dense_forward_workspace_bytes(B, K, N);
    if (!workspace || workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "dense_forward: workspace needs %zu bytes", need);
    if (misaligned(workspace, 16)) return fail(nullptr, VSTAB_E_ALIGN, "dense_forward: workspace must be 16-byte aligned");
    HIP_TRY(nullptr, launch_dense_forward(x, B, K, N, W, b, act, slope, scale, shift, y, reinterpret_cast<float *>(workspace),
                                          (hipStream_t)stream));
    return VSTAB_OK;
}
