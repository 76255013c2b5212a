// C ABI of the recurrent cells of cell.py (ConvLSTMCell :5-76, ConvGRUCell :78-136): argument checks and workspace sizes of the
// stage that follows each cell's convolution.  The kernels are in cell_ops.hip; the convolution itself is vstab_conv_forward.
#include "api_internal.h"

using namespace vstab;

namespace {

// B, H, W, F >= 1, the grid's second dimension within 65535, and a [B, H*W, stride] tensor below 2^31 elements
bool cell_shape_ok(int B, int H, int W, int F, long long stride)
{
    if (B < 1 || B > 65535 || H < 1 || W < 1 || F < 1 || stride < F) return false;
    return (long long)B * H * W * stride < (1LL << 31);
}

}  // namespace

extern "C" size_t vstab_convlstm_gates_workspace_bytes(int B, int H, int W, int F, int normalize)
{
    if (!cell_shape_ok(B, H, W, F, F)) return 0;
    return convlstm_workspace_bytes(B, H * W, F, normalize != 0);
}

extern "C" int vstab_convlstm_gates(const float *y, int ys, const float *c, const float *w_ci, const float *w_cf, const float *w_co,
                                    const float *gamma, const float *beta, int B, int H, int W, int F, float forget_bias, int act, int normalize,
                                    int peephole, float *c_out, float *h_out, float *h_cat, int cs_cat, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    if (!y || !c || !c_out || !h_out || (peephole && (!w_ci || !w_cf || !w_co)) || (normalize && (!gamma || !beta || !workspace)))
        return fail(nullptr, VSTAB_E_STATE, "convlstm_gates: NULL buffer");
    if (!cell_shape_ok(B, H, W, F, F) || !cell_shape_ok(B, H, W, F, ys) || ys < 4LL * F || act < 0 || act > 2 ||
        (h_cat && !cell_shape_ok(B, H, W, F, cs_cat)))
        return fail(nullptr, VSTAB_E_SHAPE, "convlstm_gates: need B, H, W, F >= 1, ys >= 4 F, cs_cat >= F, act 0..2 and every tensor below 2^31 elements");
    if (normalize) {
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(nullptr, VSTAB_E_ALIGN, "convlstm_gates: workspace must be 16-byte aligned");
        const size_t need = convlstm_workspace_bytes(B, H * W, F, true);
        if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "convlstm_gates: workspace %zu < %zu bytes", workspace_bytes, need);
    }
    HIP_TRY(nullptr, launch_convlstm_gates(y, ys, c, w_ci, w_cf, w_co, gamma, beta, B, H * W, F, forget_bias, act, normalize != 0, peephole != 0,
                                           c_out, h_out, h_cat, cs_cat, workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_convgru_workspace_bytes(int B, int H, int W, int F, int normalize)
{
    if (!cell_shape_ok(B, H, W, F, F)) return 0;
    return convgru_workspace_bytes(B, H * W, F, normalize != 0);
}

extern "C" int vstab_convgru_gates(const float *y, int ys, const float *h, int hs, const float *gamma, const float *beta, int B, int H, int W,
                                   int F, int normalize, float *rh, int rhs, float *u, void *workspace, size_t workspace_bytes, void *stream)
{
    if (!y || !h || !rh || !u || (normalize && (!gamma || !beta || !workspace))) return fail(nullptr, VSTAB_E_STATE, "convgru_gates: NULL buffer");
    if (!cell_shape_ok(B, H, W, F, F) || !cell_shape_ok(B, H, W, F, ys) || ys < 2LL * F || !cell_shape_ok(B, H, W, F, hs) ||
        !cell_shape_ok(B, H, W, F, rhs))
        return fail(nullptr, VSTAB_E_SHAPE, "convgru_gates: need B, H, W, F >= 1, ys >= 2 F, hs, rhs >= F and every tensor below 2^31 elements");
    if (normalize) {
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(nullptr, VSTAB_E_ALIGN, "convgru_gates: workspace must be 16-byte aligned");
        const size_t need = convgru_workspace_bytes(B, H * W, F, true);
        if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "convgru_gates: workspace %zu < %zu bytes", workspace_bytes, need);
    }
    HIP_TRY(nullptr, launch_convgru_gates(y, ys, h, hs, gamma, beta, B, H * W, F, normalize != 0, rh, rhs, u, workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_convgru_update(const float *y2, int ys, const float *h, int hs, const float *u, const float *gamma, const float *beta, int B,
                                    int H, int W, int F, int act, int normalize, float *h_out, float *h_new, int hns, void *workspace,
                                    size_t workspace_bytes, void *stream)
{
    if (!y2 || !h || !u || !h_out || (normalize && (!gamma || !beta || !workspace))) return fail(nullptr, VSTAB_E_STATE, "convgru_update: NULL buffer");
    if (!cell_shape_ok(B, H, W, F, F) || !cell_shape_ok(B, H, W, F, ys) || !cell_shape_ok(B, H, W, F, hs) || act < 0 || act > 2 ||
        (h_new && !cell_shape_ok(B, H, W, F, hns)))
        return fail(nullptr, VSTAB_E_SHAPE, "convgru_update: need B, H, W, F >= 1, ys, hs, hns >= F, act 0..2 and every tensor below 2^31 elements");
    if (normalize) {
        if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(nullptr, VSTAB_E_ALIGN, "convgru_update: workspace must be 16-byte aligned");
        const size_t need = convgru_workspace_bytes(B, H * W, F, true);
        if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "convgru_update: workspace %zu < %zu bytes", workspace_bytes, need);
    }
    HIP_TRY(nullptr, launch_convgru_update(y2, ys, h, hs, u, gamma, beta, B, H * W, F, act, normalize != 0, h_out, h_new, hns, workspace,
                                           (hipStream_t)stream));
    return VSTAB_OK;
}

// ---------------------------------------------------------------------------------------------------------------- backward
namespace {

// the checks every backward entry point shares after its own NULL / shape tests: the workspace, when the flags need one
int bwd_workspace_ok(const char *who, void *workspace, size_t workspace_bytes, size_t need)
{
    if (need == 0) return VSTAB_OK;
    if (!workspace) return fail(nullptr, VSTAB_E_STATE, "%s: NULL workspace", who);
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return fail(nullptr, VSTAB_E_ALIGN, "%s: workspace must be 16-byte aligned", who);
    if (workspace_bytes < need) return fail(nullptr, VSTAB_E_NOMEM, "%s: workspace %zu < %zu bytes", who, workspace_bytes, need);
    return VSTAB_OK;
}

}  // namespace

extern "C" size_t vstab_convlstm_gates_stats_offset(int B, int H, int W, int F, int which)
{
    if (!cell_shape_ok(B, H, W, F, F) || which < 0 || which > 1) return 0;
    return convlstm_stats_offset(B, H * W, F, which);
}

extern "C" size_t vstab_convgru_stats_offset(int B, int H, int W, int F)
{
    if (!cell_shape_ok(B, H, W, F, F)) return 0;
    return convgru_stats_offset(B, H * W, F);
}

extern "C" size_t vstab_convlstm_gates_backward_workspace_bytes(int B, int H, int W, int F, int normalize, int peephole)
{
    if (!cell_shape_ok(B, H, W, F, 10LL * F)) return 0;
    return convlstm_backward_workspace_bytes(B, H * W, F, normalize != 0, peephole != 0);
}

extern "C" int vstab_convlstm_gates_backward(const float *y, int ys, const float *c, const float *w_ci, const float *w_cf, const float *w_co,
                                             const float *gamma, const float *beta, const float *stats_jif, const float *stats_oc,
                                             const float *dh, int dhs, const float *dc_new, int B, int H, int W, int F, float forget_bias, int act,
                                             int normalize, int peephole, float *dy, int dys, float *dc, float *dw_ci, float *dw_cf,
                                             float *dw_co, float *dgamma, float *dbeta, int accumulate, void *workspace, size_t workspace_bytes,
                                             void *stream)
{
    const int npeep = (dw_ci != nullptr) + (dw_cf != nullptr) + (dw_co != nullptr);
    if (!y || !c || !dy || !dc || (peephole && (!w_ci || !w_cf || !w_co)) || (normalize && (!gamma || !beta || !stats_jif || !stats_oc)) ||
        (npeep != 0 && (npeep != 3 || !peephole)) || (!dgamma != !dbeta) || (dgamma && !normalize))
        return fail(nullptr, VSTAB_E_STATE, "convlstm_gates_backward: NULL buffer (the peephole gradients go together, as do dgamma and dbeta)");
    if (!cell_shape_ok(B, H, W, F, 10LL * F) || !cell_shape_ok(B, H, W, F, ys) || ys < 4LL * F || !cell_shape_ok(B, H, W, F, dys) || dys < 4LL * F ||
        act < 0 || act > 2 || (dh && !cell_shape_ok(B, H, W, F, dhs)))
        return fail(nullptr, VSTAB_E_SHAPE, "convlstm_gates_backward: need B, H, W, F >= 1, ys, dys >= 4 F, dhs >= F, act 0..2 and every tensor below 2^31 elements");
    const int rc = bwd_workspace_ok("convlstm_gates_backward", workspace, workspace_bytes,
                                    convlstm_backward_workspace_bytes(B, H * W, F, normalize != 0, peephole != 0));
    if (rc != VSTAB_OK) return rc;
    HIP_TRY(nullptr, launch_convlstm_gates_backward(y, ys, c, w_ci, w_cf, w_co, gamma, beta, stats_jif, stats_oc, dh, dhs, dc_new, B, H * W, F,
                                                    forget_bias, act, normalize != 0, peephole != 0, dy, dys, dc, dw_ci, dw_cf, dw_co, dgamma, dbeta,
                                                    accumulate ? 1 : 0, workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_convgru_backward_workspace_bytes(int B, int H, int W, int F, int normalize)
{
    if (!cell_shape_ok(B, H, W, F, 4LL * F)) return 0;
    return convgru_backward_workspace_bytes(B, H * W, F, normalize != 0);
}

extern "C" int vstab_convgru_update_backward(const float *y2, int ys, const float *h, int hs, const float *u, const float *gamma, const float *beta,
                                             const float *stats, const float *dh_new, int dhns, int B, int H, int W, int F, int act, int normalize,
                                             float *dy2, int dys, float *du, float *dh, int dhs, float *dgamma, float *dbeta, int accumulate,
                                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (!y2 || !h || !u || !dh_new || !dy2 || !du || !dh || (normalize && (!gamma || !beta || !stats)) || (!dgamma != !dbeta) ||
        (dgamma && !normalize))
        return fail(nullptr, VSTAB_E_STATE, "convgru_update_backward: NULL buffer (dgamma and dbeta go together)");
    if (!cell_shape_ok(B, H, W, F, 4LL * F) || !cell_shape_ok(B, H, W, F, ys) || !cell_shape_ok(B, H, W, F, hs) || !cell_shape_ok(B, H, W, F, dhns) ||
        !cell_shape_ok(B, H, W, F, dys) || !cell_shape_ok(B, H, W, F, dhs) || act < 0 || act > 2)
        return fail(nullptr, VSTAB_E_SHAPE, "convgru_update_backward: need B, H, W, F >= 1, every stride >= F, act 0..2 and every tensor below 2^31 elements");
    const int rc = bwd_workspace_ok("convgru_update_backward", workspace, workspace_bytes, convgru_backward_workspace_bytes(B, H * W, F, normalize != 0));
    if (rc != VSTAB_OK) return rc;
    HIP_TRY(nullptr, launch_convgru_update_backward(y2, ys, h, hs, u, gamma, beta, stats, dh_new, dhns, B, H * W, F, act, normalize != 0, dy2, dys, du,
                                                    dh, dhs, dgamma, dbeta, accumulate ? 1 : 0, workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_convgru_gates_backward(const float *y, int ys, const float *h, int hs, const float *gamma, const float *beta, const float *stats,
                                            const float *du, const float *drh, int drhs, int B, int H, int W, int F, int normalize, float *dy, int dys,
                                            float *dh, int dhs, float *dgamma, float *dbeta, int accumulate, void *workspace,
                                            size_t workspace_bytes, void *stream)
{
    if (!y || !h || !du || !drh || !dy || !dh || (normalize && (!gamma || !beta || !stats)) || (!dgamma != !dbeta) || (dgamma && !normalize))
        return fail(nullptr, VSTAB_E_STATE, "convgru_gates_backward: NULL buffer (dgamma and dbeta go together)");
    if (!cell_shape_ok(B, H, W, F, 4LL * F) || !cell_shape_ok(B, H, W, F, ys) || ys < 2LL * F || !cell_shape_ok(B, H, W, F, dys) || dys < 2LL * F ||
        !cell_shape_ok(B, H, W, F, hs) || !cell_shape_ok(B, H, W, F, drhs) || !cell_shape_ok(B, H, W, F, dhs))
        return fail(nullptr, VSTAB_E_SHAPE, "convgru_gates_backward: need B, H, W, F >= 1, ys, dys >= 2 F, hs, drhs, dhs >= F and every tensor below 2^31 elements");
    const int rc = bwd_workspace_ok("convgru_gates_backward", workspace, workspace_bytes, convgru_backward_workspace_bytes(B, H * W, F, normalize != 0));
    if (rc != VSTAB_OK) return rc;
    HIP_TRY(nullptr, launch_convgru_gates_backward(y, ys, h, hs, gamma, beta, stats, du, drh, drhs, B, H * W, F, normalize != 0, dy, dys, dh, dhs, dgamma,
                                                   dbeta, accumulate ? 1 : 0, workspace, (hipStream_t)stream));
    return VSTAB_OK;
}
