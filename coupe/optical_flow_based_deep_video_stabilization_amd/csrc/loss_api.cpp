// C ABI of the training objective (train_ops.hip): the per-level and the whole-pyramid loss, for one target and for many, and the test
// pass's report of it (no gradient; the scalars per level, the warped frames).
// vstab_loss_level / vstab_loss_main are the _multi entry points at one 3-channel target tensor, channel offset 0, weight 1: the
// same checks in the same order, the same kernels.
#include <cstdint>

#include "../../../include/vstab.h"
#include "api_internal.h"
#include "vstab_internal.h"

using namespace vstab;

namespace {
const int ONE_TARGET_OFF[1] = {0};
const float ONE_TARGET_WEIGHT[1] = {1.0f};

// The kernels put B in gridDim.y and index a level's [h,w,3] taps in 32-bit int.
bool loss_size_ok(int B, int h, int w) { return B >= 1 && B <= 65535 && h >= 1 && w >= 1 && (long long)h * w * 3 < (1LL << 31); }

// targets: 1..LOSS_MAX_TARGETS slices of 3 channels inside Ct
int loss_targets_check(int Ct, int T, const int *c_off, const float *weights)
{
    if (!c_off || !weights) return VSTAB_E_STATE;
    if (T < 1 || T > LOSS_MAX_TARGETS || Ct < 3) return VSTAB_E_SHAPE;
    for (int t = 0; t < T; ++t)
        if (c_off[t] < 0 || c_off[t] > Ct - 3) return VSTAB_E_SHAPE;
    return VSTAB_OK;
}

int loss_level(const char *who, const float *pf, const float *targets, int Ct, int T, const int *c_off, const float *weights,
               const float *unstab, int B, int h, int w, double *sums, float scale_mse, float scale_tv, float *grad_pf, void *stream)
{
    if (!pf || !targets || !unstab || !sums) return fail(nullptr, VSTAB_E_STATE, "%s: NULL buffer", who);
    const int c = loss_targets_check(Ct, T, c_off, weights);
    if (c == VSTAB_E_STATE) return fail(nullptr, c, "%s: NULL c_off / weights", who);
    if (c != VSTAB_OK) return fail(nullptr, c, "%s: 1..%d targets of 3 channels inside Ct, c_off[t] + 3 <= Ct", who, LOSS_MAX_TARGETS);
    if (!loss_size_ok(B, h, w)) return fail(nullptr, VSTAB_E_SHAPE, "%s: bad shape (1 <= B <= 65535, 1 <= h * w * 3 < 2^31)", who);
    if (((uintptr_t)pf | (uintptr_t)grad_pf | (uintptr_t)sums) & 7)
        return fail(nullptr, VSTAB_E_ALIGN, "%s: flow / gradient / sums must be 8-byte aligned", who);
    HIP_TRY(nullptr, launch_loss_level(pf, targets, Ct, T, c_off, weights, unstab, B, h, w, sums, scale_mse, scale_tv, grad_pf, (hipStream_t)stream));
    return VSTAB_OK;
}

int loss_main_check(const vstab_loss_level_desc *lv, int n, int B, int Ct, int T)
{
    if (!lv || n < 1 || n > 8 || B < 1) return VSTAB_E_SHAPE;
    for (int l = 0; l < n; ++l) {
        if (!lv[l].pf || lv[l].h < 1 || lv[l].w < 1 || lv[l].cs_pf < 2 || (lv[l].cs_pf & 1)) return VSTAB_E_SHAPE;
        if (lv[l].grad && (lv[l].cs_grad < 2 || (lv[l].cs_grad & 1))) return VSTAB_E_SHAPE;
        if (((uintptr_t)lv[l].pf | (uintptr_t)lv[l].grad) & 7) return VSTAB_E_ALIGN;
    }
    if (T < 1 || T > LOSS_MAX_TARGETS || Ct < 3) return VSTAB_E_SHAPE;
    for (int l = 0; l < n; ++l)
        if (!loss_size_ok(B, lv[l].h, lv[l].w)) return VSTAB_E_SHAPE;
    return VSTAB_OK;
}

size_t loss_main_bytes(const vstab_loss_level_desc *levels, int n_levels, int B, int Ct, int T)
{
    if (loss_main_check(levels, n_levels, B, Ct, T) != VSTAB_OK) return 0;
    static_assert(sizeof(vstab_loss_level_desc) == sizeof(LossLevel), "descriptor layout");
    return loss_main_workspace_bytes(B, reinterpret_cast<const LossLevel *>(levels), n_levels, Ct, T);
}

// what vstab_loss_report adds to a loss_main call: the levels' previews and their type
struct LossReportArgs { void *const *previews; int preview_dtype; };

int loss_main(const char *who, const vstab_loss_level_desc *levels, int n_levels, const float *targets, int Ct, int T, const int *c_off,
              const float *weights, const float *unstab, int B, int H, int W, double *loss_out, bool per_target, void *workspace,
              size_t workspace_bytes, void *stream, const LossReportArgs *report = nullptr)
{
    int c = loss_main_check(levels, n_levels, B, Ct, T);
    if (c != VSTAB_OK)
        return fail(nullptr, c, "%s: bad level descriptor or target count (1..8 levels of h * w * 3 < 2^31, B <= 65535, even channel strides >= 2, "
                                "8-byte aligned buffers, 1..%d targets, Ct >= 3)", who, LOSS_MAX_TARGETS);
    if (!targets || !unstab || !loss_out || !workspace) return fail(nullptr, VSTAB_E_STATE, "%s: NULL buffer", who);
    c = loss_targets_check(Ct, T, c_off, weights);
    if (c == VSTAB_E_STATE) return fail(nullptr, c, "%s: NULL c_off / weights", who);
    if (c != VSTAB_OK) return fail(nullptr, c, "%s: every target needs 0 <= c_off[t] and c_off[t] + 3 <= Ct", who);
    if (H < 1 || W < 1) return fail(nullptr, VSTAB_E_SHAPE, "%s: bad image shape", who);
    if (((uintptr_t)loss_out | (uintptr_t)workspace) & 7) return fail(nullptr, VSTAB_E_ALIGN, "%s: loss_out / workspace must be 8-byte aligned", who);
    const LossLevel *lv = reinterpret_cast<const LossLevel *>(levels);
    if (workspace_bytes < loss_main_workspace_bytes(B, lv, n_levels, Ct, T)) return fail(nullptr, VSTAB_E_NOMEM, "%s: workspace too small", who);
    void *ws = (void *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    if (report) {
        if (report->preview_dtype != 0 && report->preview_dtype != 1)
            return fail(nullptr, VSTAB_E_SHAPE, "%s: preview_dtype must be 0 (float32) or 1 (uint8)", who);
        for (int l = 0; report->previews && report->preview_dtype == 0 && l < n_levels; ++l)
            if ((uintptr_t)report->previews[l] & 3) return fail(nullptr, VSTAB_E_ALIGN, "%s: a float32 preview must be 4-byte aligned", who);
        HIP_TRY(nullptr, launch_loss_report(lv, n_levels, targets, Ct, T, c_off, weights, unstab, B, H, W, report->previews,
                                            report->preview_dtype == 1, loss_out, ws, (hipStream_t)stream));
        return VSTAB_OK;
    }
    HIP_TRY(nullptr, launch_loss_main(lv, n_levels, targets, Ct, T, c_off, weights, unstab, B, H, W, loss_out, per_target, ws, (hipStream_t)stream));
    return VSTAB_OK;
}

// The report writes no gradient and ignores levels[l].grad: the descriptors as loss_main's checks should see them, grad NULL.  An
// array or count the checks refuse anyway is handed through as it is.
struct GradlessLevels {
    vstab_loss_level_desc copy[8];
    const vstab_loss_level_desc *lv;
    GradlessLevels(const vstab_loss_level_desc *levels, int n) : lv(levels)
    {
        if (!levels || n < 1 || n > 8) return;
        for (int l = 0; l < n; ++l) { copy[l] = levels[l]; copy[l].grad = nullptr; copy[l].cs_grad = 0; }
        lv = copy;
    }
};
}  // namespace

extern "C" int vstab_loss_level(const float *pf, const float *gt, const float *unstab, int B, int h, int w, double *sums,
                                float scale_mse, float scale_tv, float *grad_pf, void *stream)
{
    return loss_level("loss_level", pf, gt, 3, 1, ONE_TARGET_OFF, ONE_TARGET_WEIGHT, unstab, B, h, w, sums, scale_mse, scale_tv, grad_pf, stream);
}

extern "C" int vstab_loss_level_multi(const float *pf, const float *targets, int Ct, int T, const int *c_off, const float *weights,
                                      const float *unstab, int B, int h, int w, double *sums, float scale_tv, float *grad_pf, void *stream)
{
    return loss_level("loss_level_multi", pf, targets, Ct, T, c_off, weights, unstab, B, h, w, sums, 1.0f, scale_tv, grad_pf, stream);
}

extern "C" size_t vstab_loss_main_workspace_bytes(const vstab_loss_level_desc *levels, int n_levels, int B)
{
    return loss_main_bytes(levels, n_levels, B, 3, 1);
}

// loss_out: one double
extern "C" int vstab_loss_main(const vstab_loss_level_desc *levels, int n_levels, const float *gtstab, const float *unstab, int B, int H,
                               int W, double *loss_out, void *workspace, size_t workspace_bytes, void *stream)
{
    return loss_main("loss_main", levels, n_levels, gtstab, 3, 1, ONE_TARGET_OFF, ONE_TARGET_WEIGHT, unstab, B, H, W, loss_out, false, workspace,
                     workspace_bytes, stream);
}

extern "C" size_t vstab_loss_main_multi_workspace_bytes(const vstab_loss_level_desc *levels, int n_levels, int B, int Ct, int T)
{
    return loss_main_bytes(levels, n_levels, B, Ct, T);
}

// loss_out: 1 + T doubles
extern "C" int vstab_loss_main_multi(const vstab_loss_level_desc *levels, int n_levels, const float *targets, int Ct, int T, const int *c_off,
                                     const float *weights, const float *unstab, int B, int H, int W, double *loss_out, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    return loss_main("loss_main_multi", levels, n_levels, targets, Ct, T, c_off, weights, unstab, B, H, W, loss_out, true, workspace,
                     workspace_bytes, stream);
}

// ---- the test pass's loss report (main:277-326, 346-372): loss_main_multi's checks in its order, then the previews'
extern "C" size_t vstab_loss_report_workspace_bytes(const vstab_loss_level_desc *levels, int n_levels, int B, int Ct, int T)
{
    return loss_main_bytes(GradlessLevels(levels, n_levels).lv, n_levels, B, Ct, T);
}

// out: 1 + T + 2 * n_levels doubles
extern "C" int vstab_loss_report(const vstab_loss_level_desc *levels, int n_levels, const float *targets, int Ct, int T, const int *c_off,
                                 const float *weights, const float *unstab, int B, int H, int W, void *const *previews, int preview_dtype,
                                 double *out, void *workspace, size_t workspace_bytes, void *stream)
{
    const LossReportArgs report = {previews, preview_dtype};
    return loss_main("loss_report", GradlessLevels(levels, n_levels).lv, n_levels, targets, Ct, T, c_off, weights, unstab, B, H, W, out, true,
                     workspace, workspace_bytes, stream, &report);
}
