// C ABI of the training step's elementwise and reduction blocks: BatchNorm in training mode, the resamplers'
// adjoints, Adam, column sums, the full-resolution head's tap tables.  The objective is in loss_api.cpp, the convolutions and their
// gradients in train_conv_api.cpp.
#include <cstdint>

#include "../../../include/vstab.h"
#include "api_internal.h"
#include "vstab_internal.h"

using namespace vstab;

// ------------------------------------------------------------------------- BatchNorm (training and inference mode) + leaky relu
extern "C" size_t vstab_bn_scratch_bytes(long long rows, int C)
{
    if (rows < 1 || C < 1) return 0;
    return ((size_t)4 * bn_chunks(rows, C) + 2) * C * sizeof(float) + 256;
}

extern "C" int vstab_bn_lrelu_train_forward(float *zy, long long rows, int cs, int c_off, int C, const float *beta, float *moving_mean,
                                            float *moving_var, float decay, float eps, float *save_mean, float *save_rstd, void *scratch,
                                            size_t scratch_bytes, void *stream)
{
    if (!zy || !beta || !save_mean || !save_rstd || !scratch) return fail(nullptr, VSTAB_E_STATE, "bn_lrelu_train_forward: NULL buffer");
    if (rows < 1 || C < 1 || c_off < 0 || c_off + C > cs) return fail(nullptr, VSTAB_E_SHAPE, "bn_lrelu_train_forward: bad shape");
    if ((C & 3) || (cs & 3) || (c_off & 3) || (reinterpret_cast<uintptr_t>(zy) & 15) || (reinterpret_cast<uintptr_t>(beta) & 15) ||
        (reinterpret_cast<uintptr_t>(save_mean) & 15) || (reinterpret_cast<uintptr_t>(save_rstd) & 15))
        return fail(nullptr, VSTAB_E_ALIGN, "bn_lrelu_train_forward: channels multiples of 4, 16-byte aligned buffers");
    if (scratch_bytes < vstab_bn_scratch_bytes(rows, C)) return fail(nullptr, VSTAB_E_NOMEM, "bn_lrelu_train_forward: scratch too small");
    HIP_TRY(nullptr, launch_bn_lrelu_train_forward(zy, rows, cs, c_off, C, beta, moving_mean, moving_var, decay, eps, save_mean, save_rstd,
                                                   reinterpret_cast<float *>(scratch), (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_bn_lrelu_inference_forward(float *zy, long long rows, int cs, int c_off, int C, const float *beta, const float *moving_mean,
                                                const float *moving_var, float eps, void *stream)
{
    if (!zy || !beta || !moving_mean || !moving_var) return fail(nullptr, VSTAB_E_STATE, "bn_lrelu_inference_forward: NULL buffer");
    if (rows < 1 || C < 1 || c_off < 0 || c_off + C > cs) return fail(nullptr, VSTAB_E_SHAPE, "bn_lrelu_inference_forward: bad shape");
    if ((C & 3) || (cs & 3) || (c_off & 3) || (reinterpret_cast<uintptr_t>(zy) & 15) || (reinterpret_cast<uintptr_t>(beta) & 15) ||
        (reinterpret_cast<uintptr_t>(moving_mean) & 15) || (reinterpret_cast<uintptr_t>(moving_var) & 15))
        return fail(nullptr, VSTAB_E_ALIGN, "bn_lrelu_inference_forward: channels multiples of 4, 16-byte aligned buffers");
    HIP_TRY(nullptr, launch_bn_lrelu_inference_forward(zy, rows, cs, c_off, C, beta, moving_mean, moving_var, eps, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_bn_lrelu_train_backward(const float *y, int cs_y, int cy_off, float *dy, int cs_g, int cg_off, int C, long long rows,
                                             const float *beta, const float *save_rstd, float *dbeta, int accumulate, void *scratch,
                                             size_t scratch_bytes, void *stream)
{
    if (!y || !dy || !beta || !save_rstd || !scratch) return fail(nullptr, VSTAB_E_STATE, "bn_lrelu_train_backward: NULL buffer");
    if (rows < 1 || C < 1 || cy_off < 0 || cg_off < 0 || cy_off + C > cs_y || cg_off + C > cs_g)
        return fail(nullptr, VSTAB_E_SHAPE, "bn_lrelu_train_backward: bad shape");
    if (scratch_bytes < vstab_bn_scratch_bytes(rows, C)) return fail(nullptr, VSTAB_E_NOMEM, "bn_lrelu_train_backward: scratch too small");
    HIP_TRY(nullptr, launch_bn_lrelu_train_backward(y, cs_y, cy_off, dy, cs_g, cg_off, C, rows, beta, save_rstd, dbeta, accumulate ? 1 : 0,
                                                    reinterpret_cast<float *>(scratch), (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_lrelu_backward(const float *y, int cs_y, int cy_off, float *dy, int cs_g, int cg_off, int C, long long rows, void *stream)
{
    if (!y || !dy) return fail(nullptr, VSTAB_E_STATE, "lrelu_backward: NULL buffer");
    if (rows < 1 || C < 1 || cy_off < 0 || cg_off < 0 || cy_off + C > cs_y || cg_off + C > cs_g)
        return fail(nullptr, VSTAB_E_SHAPE, "lrelu_backward: bad shape");
    HIP_TRY(nullptr, launch_lrelu_backward(y, cs_y, cy_off, dy, cs_g, cg_off, C, rows, (hipStream_t)stream));
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- resampler adjoints, full-res upsampler, Adam
extern "C" int vstab_resize_bilinear_backward(const float *dout, int B, int oh, int ow, int C, float *din, int h, int w, float gain,
                                              int accumulate, void *stream)
{
    if (!dout || !din) return fail(nullptr, VSTAB_E_STATE, "resize_bilinear_backward: NULL buffer");
    if (B < 1 || oh < 1 || ow < 1 || h < 1 || w < 1 || C < 1) return fail(nullptr, VSTAB_E_SHAPE, "resize_bilinear_backward: bad shape");
    HIP_TRY(nullptr, launch_resize_bilinear_backward(dout, B, oh, ow, C, din, h, w, gain, accumulate ? 1 : 0, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_pad_nearest_upsample(const float *src, int B, int h2, int w2, int C, float *out, int H, int W, void *stream)
{
    if (!src || !out) return fail(nullptr, VSTAB_E_STATE, "pad_nearest_upsample: NULL buffer");
    if (B < 1 || h2 < 1 || w2 < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return fail(nullptr, VSTAB_E_SHAPE, "pad_nearest_upsample: bad shape");
    if ((long long)B * H * W * C * 4 >= (1LL << 40)) return fail(nullptr, VSTAB_E_SHAPE, "pad_nearest_upsample: too large");
    HIP_TRY(nullptr, launch_pad_nearest_up(src, B, h2, w2, C, out, H, W, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_pad_nearest_upsample_backward(const float *dout, int B, int H, int W, int C, float *dsrc, int h2, int w2, int accumulate,
                                                   void *stream)
{
    if (!dout || !dsrc) return fail(nullptr, VSTAB_E_STATE, "pad_nearest_upsample_backward: NULL buffer");
    if (B < 1 || h2 < 1 || w2 < 1 || H < 1 || W < 1 || C < 4 || (C & 3))
        return fail(nullptr, VSTAB_E_SHAPE, "pad_nearest_upsample_backward: bad shape");
    HIP_TRY(nullptr, launch_pad_nearest_up_backward(dout, B, H, W, C, dsrc, h2, w2, accumulate ? 1 : 0, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_adam_step(float *w, const float *g, float *m, float *v, long long n, float lr_t, float beta1, float beta2, float eps,
                               void *stream)
{
    if (!w || !g || !m || !v) return fail(nullptr, VSTAB_E_STATE, "adam_step: NULL buffer");
    if (n < 1) return fail(nullptr, VSTAB_E_SHAPE, "adam_step: bad size");
    HIP_TRY(nullptr, launch_adam(w, g, m, v, n, lr_t, beta1, beta2, eps, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_column_sum_scratch_bytes(long long rows, int C) { return rows < 1 || C < 1 ? 0 : (size_t)column_sum_chunks(rows, C) * C * sizeof(float) + 256; }

extern "C" int vstab_column_sum(const float *g, long long rows, int cs, int c_off, int C, float *out, int accumulate, void *scratch,
                                size_t scratch_bytes, void *stream)
{
    if (!g || !out || !scratch) return fail(nullptr, VSTAB_E_STATE, "column_sum: NULL buffer");
    if (rows < 1 || C < 1 || c_off < 0 || c_off + C > cs) return fail(nullptr, VSTAB_E_SHAPE, "column_sum: bad shape");
    if (scratch_bytes < vstab_column_sum_scratch_bytes(rows, C)) return fail(nullptr, VSTAB_E_NOMEM, "column_sum: scratch too small");
    HIP_TRY(nullptr, launch_column_sum(g, rows, cs, c_off, C, out, accumulate ? 1 : 0, reinterpret_cast<float *>(scratch), (hipStream_t)stream));
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- full-resolution head through its tap table
extern "C" int vstab_pf2_from_taps(const float *T, int B, int h2, int w2, const float *bias2, const float *pf3, int h3, int w3, float *pf2,
                                   int H, int W, void *stream)
{
    if (!T || !bias2 || !pf3 || !pf2) return fail(nullptr, VSTAB_E_STATE, "pf2_from_taps: NULL buffer");
    if (B < 1 || h2 < 1 || w2 < 1 || h3 < 1 || w3 < 1 || H < 3 || W < 3) return fail(nullptr, VSTAB_E_SHAPE, "pf2_from_taps: bad shape");
    HIP_TRY(nullptr, launch_pf2(T, B, h2, w2, bias2, pf3, h3, w3, pf2, H, W, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_predict2_tap_table(const float *concat2, long long M, const float *table, float *T, void *stream)
{
    if (!concat2 || !table || !T) return fail(nullptr, VSTAB_E_STATE, "predict2_tap_table: NULL buffer");
    if (M < 1 || M * 784 >= 0x80000000LL) return fail(nullptr, VSTAB_E_SHAPE, "predict2_tap_table: 1 <= M, M * 784 < 2^31");
    if (((uintptr_t)concat2 | (uintptr_t)T | (uintptr_t)table) & 15) return fail(nullptr, VSTAB_E_ALIGN, "predict2_tap_table: buffers must be 16-byte aligned");
    static const hipError_t attr = tap_panel_set_attributes();
    HIP_TRY(nullptr, attr);
    HIP_TRY(nullptr, launch_tap_panel(concat2, M, table, T, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_pf2_taps_backward(const float *g, int cs_g, int B, int H, int W, float *dT, int h2, int w2, void *stream)
{
    if (!g || !dT) return fail(nullptr, VSTAB_E_STATE, "pf2_taps_backward: NULL buffer");
    if (B < 1 || h2 < 1 || w2 < 1 || H < 3 || W < 3 || cs_g < 2) return fail(nullptr, VSTAB_E_SHAPE, "pf2_taps_backward: bad shape");
    HIP_TRY(nullptr, launch_pf2_taps_backward(g, cs_g, B, H, W, dT, h2, w2, (hipStream_t)stream));
    return VSTAB_OK;
}
