// C ABI of the NLDF saliency head's backward (NLDF.py: Model.backward / pools_grad): the reverse walk of
// vstab_nldf_forward from the gradient at Score down to the five pools and the 30 variables, and thin entries to its own kernels.
// No arithmetic here: the Score stage, the contrast adjoint and the gates are nldf_grad_ops.hip, every convolution gradient goes
// through the training convolutions' entry points (train_conv_api.cpp) on the raw variables vstab_nldf_load keeps.
#include <algorithm>

#include "api_internal.h"
#include "nldf_plan.h"

using namespace vstab;
using namespace nldf;

namespace {

constexpr int NPIX = 176 * 176;
constexpr int LF_C = 5 * FEA;                   // Local_Fea channels
constexpr int LF_WGRAD_CHUNKS = 8;              // Local_Fea's filter gradient: calls per sample ...
constexpr int LF_WGRAD_ROWS = NPIX / LF_WGRAD_CHUNKS;      // ... of this many pixel rows each
static_assert(LF_WGRAD_ROWS * LF_WGRAD_CHUNKS == NPIX, "the chunks cover a sample");

// The backward's own workspace: gradient buffers of the concat tensors, of Local_Fea and of the global branch, the Score stage's
// partial sums, then the scratch of whichever launcher is at work.
enum BBuf { D_CAT1, D_CAT2, D_CAT3, D_CAT4, D_CAT5, D_LF, D_LS, D_G1, D_G2, D_FG, D_GS, D_PART, D_LSW, D_TMPW, D_NBUF };

struct BwdPlan { size_t off[D_NBUF], scratch_off, scratch, total; };

// scratch of the Score stage alone: the pixel-sum slabs and the Local_Score filter gradient's slabs
size_t score_part_bytes(int B) { return a256(nldf_score_part_floats(B) * sizeof(float)); }
size_t score_lsw_bytes() { return a256(local_score_wgrad_scratch_floats(LF_C) * sizeof(float)); }

bool bwd_plan(int B, bool need_weights, BwdPlan &bp)
{
    NldfPlan pl;
    if (!nldf_plan(B, pl)) return false;
    size_t n[D_NBUF];
    for (int k = 0; k < 5; ++k) n[D_CAT1 + k] = (size_t)B * POOL_HW[k] * POOL_HW[k] * CAT_C[k] * 4;
    n[D_LF] = (size_t)B * NPIX * LF_C * 4;
    n[D_LS] = (size_t)B * NPIX * 2 * 4;
    n[D_G1] = (size_t)B * 49 * FEA * 4;
    n[D_G2] = (size_t)B * 9 * FEA * 4;
    n[D_FG] = (size_t)B * FEA * 4;
    n[D_GS] = (size_t)B * 2 * 4;
    n[D_PART] = score_part_bytes(B);
    n[D_LSW] = score_lsw_bytes();
    // a filter gradient that runs as several calls adds them up here when it has to be ADDED to the caller's: one rounding, as a single call
    n[D_TMPW] = need_weights ? (size_t)25 * UP_C[0] * CAT_C[1] * 4 : 0;
    size_t off = 0;
    for (int i = 0; i < D_NBUF; ++i) { bp.off[i] = off; off += a256(n[i]); }
    // the launchers' scratch: the largest any of them asks for (0 from a query = that launcher refuses the geometry)
    size_t s = 256;
    bool ok = true;
    auto take = [&](size_t v) { if (v == 0) ok = false; s = std::max(s, v); };
    take(vstab_conv_dgrad_workspace_bytes(B, 176, 176, LF_C, LF_C, 1, 1, 0, 176, 176, CAT_C[0], 0, CAT_C[0], 0));
    if (need_weights) {
        take(vstab_conv_wgrad_workspace_bytes(1, LF_WGRAD_ROWS, 1, 1, CAT_C[0], LF_C));
        take(vstab_column_sum_scratch_bytes((long long)B * NPIX, LF_C));
    }
    for (int k = 0; k < 4; ++k) {
        const int h = POOL_HW[k], h2 = POOL_HW[k + 1];
        take(vstab_conv_forward_workspace_bytes(B, h, h, CAT_C[k], UP_C[k], 5, 2, 1, CAT_C[k + 1], CAT_C[k + 1], 0, 0, h2, h2));
        take(vstab_column_sum_scratch_bytes((long long)B * h * h, UP_C[k]));
        if (need_weights) take(vstab_conv_wgrad_workspace_bytes(1, h2, h2, 5, UP_C[k], CAT_C[k + 1]));
    }
    for (int k = 0; k < 5; ++k) {
        const int h = POOL_HW[k];
        take(vstab_conv_dgrad_workspace_bytes(B, h, h, CAT_C[k], FEA, 3, 1, 1, h, h, POOL_C[k], 0, POOL_C[k], k == 4 ? 1 : 0));
        if (need_weights) take(vstab_conv_wgrad_workspace_bytes(B, h, h, 3, POOL_C[k], FEA));
    }
    take(vstab_conv_dgrad_workspace_bytes(B, 1, 1, FEA, FEA, 3, 1, 0, 3, 3, FEA, 0, FEA, 0));
    take(vstab_conv_dgrad_workspace_bytes(B, 3, 3, FEA, FEA, 5, 1, 0, 7, 7, FEA, 0, FEA, 0));
    take(vstab_conv_dgrad_workspace_bytes(B, 7, 7, FEA, FEA, 5, 1, 0, 11, 11, 512, 0, 512, 0));
    if (need_weights) {
        take(vstab_conv_wgrad_workspace_bytes(B, 1, 1, 3, FEA, FEA));
        take(vstab_conv_wgrad_workspace_bytes(B, 3, 3, 5, FEA, FEA));
        take(vstab_conv_wgrad_workspace_bytes(B, 7, 7, 5, 512, FEA));
    }
    if (!ok) return false;
    bp.scratch_off = off;
    bp.scratch = a256(s);
    bp.total = off + bp.scratch;
    return true;
}

}  // namespace

extern "C" size_t vstab_nldf_backward_workspace_bytes(int B, int need_weights)
{
    BwdPlan bp;
    if (!bwd_plan(B, need_weights != 0, bp)) { fail(nullptr, VSTAB_E_SHAPE, "nldf_backward: unsupported batch %d", B); return 0; }
    return bp.total;
}

extern "C" int vstab_nldf_backward(vstab_ctx *ctx, const float *const *pools5, int B, const void *fwd_workspace, size_t fwd_workspace_bytes,
                                   const float *local_fea, const float *prob, const float *dscore, const float *dprob, const float *dlocal_fea,
                                   const float *dfea_global, float *const *dpools5, float *const *dparams, int accumulate_params,
                                   void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "nldf_backward: ctx is NULL");
    vstab_nldf *N = static_cast<vstab_nldf *>(ctx->nldf);
    if (!N || !N->loaded) return fail(ctx, VSTAB_E_STATE, "nldf_backward: vstab_nldf_load has not been called");
    if (!pools5 || !fwd_workspace || !local_fea || !dscore || !workspace) return fail(ctx, VSTAB_E_STATE, "nldf_backward: NULL buffer");
    if (dprob && !prob) return fail(ctx, VSTAB_E_STATE, "nldf_backward: dprob needs prob");
    for (int k = 0; k < 5; ++k)
        if (!pools5[k]) return fail(ctx, VSTAB_E_STATE, "nldf_backward: pool%d is NULL", k + 1);
    auto W_of = [&](int l) { return dparams ? dparams[2 * l] : nullptr; };
    auto b_of = [&](int l) { return dparams ? dparams[2 * l + 1] : nullptr; };
    bool any_param = false, any_pool = false;
    for (int l = 0; l < L_COUNT; ++l) {
        if (b_of(l) && !W_of(l)) return fail(ctx, VSTAB_E_STATE, "nldf_backward: layer %d: a bias gradient without its filter gradient", l);
        any_param = any_param || W_of(l);
    }
    for (int k = 0; k < 5; ++k) any_pool = any_pool || (dpools5 && dpools5[k]);
    if (!any_param && !any_pool) return fail(ctx, VSTAB_E_STATE, "nldf_backward: neither a pool gradient nor a parameter gradient is asked for");
    uintptr_t bits = (uintptr_t)local_fea | (uintptr_t)prob | (uintptr_t)dscore | (uintptr_t)dprob | (uintptr_t)dlocal_fea | (uintptr_t)dfea_global;
    for (int k = 0; k < 5; ++k) bits |= (uintptr_t)pools5[k] | (uintptr_t)(dpools5 ? dpools5[k] : nullptr);
    if (dparams) for (int i = 0; i < 2 * L_COUNT; ++i) bits |= (uintptr_t)dparams[i];
    if (bits & 15) return fail(ctx, VSTAB_E_ALIGN, "nldf_backward: every tensor must be 16-byte aligned");
    if (((uintptr_t)fwd_workspace | (uintptr_t)workspace) & 255) return fail(ctx, VSTAB_E_ALIGN, "nldf_backward: workspaces must be 256-byte aligned");
    NldfPlan pl;
    if (!nldf_plan(B, pl)) return fail(ctx, VSTAB_E_SHAPE, "nldf_backward: unsupported batch %d", B);
    if (fwd_workspace_bytes < pl.total) return fail(ctx, VSTAB_E_NOMEM, "nldf_backward: forward workspace %zu < %zu bytes", fwd_workspace_bytes, pl.total);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    BwdPlan bp;
    if (!bwd_plan(B, any_param, bp)) return fail(ctx, VSTAB_E_SHAPE, "nldf_backward: unsupported batch %d", B);
    if (workspace_bytes < bp.total) return fail(ctx, VSTAB_E_NOMEM, "nldf_backward: workspace %zu < %zu bytes", workspace_bytes, bp.total);

    hipStream_t stream = (hipStream_t)stream_;
    const char *fws = static_cast<const char *>(fwd_workspace);
    char *ws = static_cast<char *>(workspace);
    auto fbuf = [&](int b) { return reinterpret_cast<const float *>(fws + pl.off[b]); };
    auto buf = [&](int b) { return reinterpret_cast<float *>(ws + bp.off[b]); };
    void *scratch = ws + bp.scratch_off;
    const float *w = N->w;
    const NldfWeights &o = N->o;
    const int acc = accumulate_params ? 1 : 0;
    const int cat_buf[5] = {N_CAT1, N_CAT2, N_CAT3, N_CAT4, N_CAT5};
    float *dpool[5];
    for (int k = 0; k < 5; ++k) dpool[k] = dpools5 ? dpools5[k] : nullptr;
#define GEN(call) do { if (const int c_ = (call)) { adopt_last_error(ctx); return c_; } } while (0)

    // what has to be computed: level k (0..4) wants its gated Fea_P gradient; `deeper[k]`: something below cat(k+1)'s Up slice
    bool want_level[5], deeper[5];
    for (int k = 0; k < 5; ++k) want_level[k] = dpool[k] || W_of(L_P1 + k);
    deeper[4] = false;
    for (int k = 3; k >= 0; --k) deeper[k] = deeper[k + 1] || want_level[k + 1] || W_of(deconv_layer(k));
    const bool below_cat1 = deeper[0] || want_level[0];
    const bool need_dlf = below_cat1 || W_of(L_LF);
    const bool need_g2 = dpool[4] || W_of(L_G1) || W_of(L_G2);        // is the gradient at G2 needed?
    const bool need_g1 = dpool[4] || W_of(L_G1);

    // ---- Score stage: Local_Score's gradient, Global_Score's (per-sample pixel sums), both biases, Global_Score's layer
    const float *dls = dprob ? buf(D_LS) : dscore;
    HIP_TRY(ctx, launch_nldf_score_grad(dscore, prob, dprob, B, NPIX, buf(D_LS), buf(D_PART), stream));
    HIP_TRY(ctx, launch_nldf_score_fold(buf(D_PART), B, fbuf(N_G), w + o.raw_w[L_GS], dfea_global, buf(D_GS), buf(D_FG), W_of(L_GS), b_of(L_GS),
                                        b_of(L_LS), acc, stream));
    if (W_of(L_LS)) HIP_TRY(ctx, launch_local_score_wgrad(local_fea, dls, (long long)B * NPIX, LF_C, W_of(L_LS), acc, buf(D_LSW), stream));
    if (need_dlf) HIP_TRY(ctx, launch_local_score_dgrad(dls, w + o.raw_w[L_LS], (long long)B * NPIX, LF_C, dlocal_fea, buf(D_LF), stream));

    // ---- global branch (VALID convolutions 11 -> 7 -> 3 -> 1 on pool5): writes dpool5, which Fea_P5's input gradient then adds to
    if (W_of(L_G)) GEN(vstab_conv_wgrad(fbuf(N_G2), B, 3, 3, FEA, 0, FEA, buf(D_FG), 1, 1, FEA, 0, FEA, 3, 1, 0, W_of(L_G), b_of(L_G), acc, scratch, bp.scratch, stream));
    if (need_g2) {
        GEN(vstab_conv_dgrad(buf(D_FG), B, 1, 1, FEA, 0, FEA, w + o.raw_w[L_G], nullptr, 3, 1, 0, buf(D_G2), 3, 3, FEA, 0, FEA, 0, scratch, bp.scratch, stream));
        HIP_TRY(ctx, launch_relu_backward(fbuf(N_G2), buf(D_G2), (long long)B * 9 * FEA / 4, stream));
        if (W_of(L_G2)) GEN(vstab_conv_wgrad(fbuf(N_G1), B, 7, 7, FEA, 0, FEA, buf(D_G2), 3, 3, FEA, 0, FEA, 5, 1, 0, W_of(L_G2), b_of(L_G2), acc, scratch, bp.scratch, stream));
    }
    if (need_g1) {
        GEN(vstab_conv_dgrad(buf(D_G2), B, 3, 3, FEA, 0, FEA, w + o.raw_w[L_G2], nullptr, 5, 1, 0, buf(D_G1), 7, 7, FEA, 0, FEA, 0, scratch, bp.scratch, stream));
        HIP_TRY(ctx, launch_relu_backward(fbuf(N_G1), buf(D_G1), (long long)B * 49 * FEA / 4, stream));
        if (W_of(L_G1)) GEN(vstab_conv_wgrad(pools5[4], B, 11, 11, 512, 0, 512, buf(D_G1), 7, 7, FEA, 0, FEA, 5, 1, 0, W_of(L_G1), b_of(L_G1), acc, scratch, bp.scratch, stream));
        if (dpool[4]) GEN(vstab_conv_dgrad(buf(D_G1), B, 7, 7, FEA, 0, FEA, w + o.raw_w[L_G1], nullptr, 5, 1, 0, dpool[4], 11, 11, 512, 0, 512, 0, scratch, bp.scratch, stream));
    }

    // ---- Local_Fea (1x1, 768 -> 640)
    if (W_of(L_LF)) {
        // A 1x1 layer's filter gradient is a plain reduction over the B * 176 * 176 pixel rows, so the rows may be cut anywhere: it runs
        // as LF_WGRAD_CHUNKS calls per sample that add into dW.  One call would sum 30976 B rows in 17 split-K chains of 1800 B float32
        // additions each; the pieces keep every chain near 230 additions, which is where the result's last bits come from (section 22).
        float *dW = acc ? buf(D_TMPW) : W_of(L_LF);
        for (int c = 0; c < B * LF_WGRAD_CHUNKS; ++c) {
            const size_t row0 = (size_t)c * LF_WGRAD_ROWS;
            GEN(vstab_conv_wgrad(fbuf(N_CAT1) + row0 * CAT_C[0], 1, LF_WGRAD_ROWS, 1, CAT_C[0], 0, CAT_C[0], buf(D_LF) + row0 * LF_C, LF_WGRAD_ROWS, 1, LF_C,
                                 0, LF_C, 1, 1, 0, dW, nullptr, c > 0 ? 1 : 0, scratch, bp.scratch, stream));
        }
        if (acc) HIP_TRY(ctx, launch_axpby(W_of(L_LF), 1.f, dW, 1.f, W_of(L_LF), (long long)CAT_C[0] * LF_C, stream));
        if (b_of(L_LF)) HIP_TRY(ctx, launch_column_sum(buf(D_LF), (long long)B * NPIX, LF_C, 0, LF_C, b_of(L_LF), acc, static_cast<float *>(scratch), stream));
    }
    if (below_cat1) GEN(vstab_conv_dgrad(buf(D_LF), B, 176, 176, LF_C, 0, LF_C, w + o.raw_w[L_LF], nullptr, 1, 1, 0, buf(D_CAT1), 176, 176, CAT_C[0], 0, CAT_C[0], 0, scratch, bp.scratch, stream));

    // ---- levels: dcat_k = [dP | dLC | dUp]
    for (int k = 0; k < 5 && (k == 0 ? below_cat1 : deeper[k - 1]); ++k) {
        const int h = POOL_HW[k], cs = CAT_C[k];
        const float *cat = fbuf(cat_buf[k]);
        float *dcat = buf(D_CAT1 + k);
        if (k < 4 && deeper[k]) {
            // Up slice: gate by Up > 0, its column sum is the transposed conv's bias gradient; the transposed conv's input gradient is
            // the stride-2 SAME convolution of the gated slice with W read as HWIO (I = its output, O = its input channels)
            const int l = deconv_layer(k), h2 = POOL_HW[k + 1], cs2 = CAT_C[k + 1];
            HIP_TRY(ctx, launch_slice_gate(cat, dcat, (long long)B * h * h, cs, 2 * FEA, UP_C[k], stream));
            if (b_of(l)) HIP_TRY(ctx, launch_column_sum(dcat, (long long)B * h * h, cs, 2 * FEA, UP_C[k], b_of(l), acc, static_cast<float *>(scratch), stream));
            // one call per sample, adding into dW: the launcher does not split this reduction (12800 x 640 outputs fill the chip), so a
            // call over the batch would sum B * h2 * h2 pixels in ONE float32 chain per element
            if (W_of(l)) {
                const bool via_tmp = acc && B > 1;
                float *dW = via_tmp ? buf(D_TMPW) : W_of(l);
                for (int n = 0; n < B; ++n)
                    GEN(vstab_conv_wgrad(dcat + (size_t)n * h * h * cs, 1, h, h, cs, 2 * FEA, UP_C[k], fbuf(cat_buf[k + 1]) + (size_t)n * h2 * h2 * cs2, h2, h2, cs2, 0,
                                         cs2, 5, 2, 1, dW, nullptr, (n > 0 || (acc && !via_tmp)) ? 1 : 0, scratch, bp.scratch, stream));
                if (via_tmp) HIP_TRY(ctx, launch_axpby(W_of(l), 1.f, dW, 1.f, W_of(l), (long long)25 * UP_C[k] * cs2, stream));
            }
            if (deeper[k + 1] || want_level[k + 1])
                GEN(vstab_conv_forward(dcat, B, h, h, cs, 2 * FEA, UP_C[k], w + o.raw_w[l], nullptr, 5, 2, 1, buf(D_CAT1 + k + 1), h2, h2, cs2, 0, cs2, 0, scratch, bp.scratch, stream));
        }
        if (want_level[k]) {
            HIP_TRY(ctx, launch_contrast_gate_backward(cat, dcat, B, h, h, FEA, cs, stream));
            const int l = L_P1 + k;
            if (W_of(l)) GEN(vstab_conv_wgrad(pools5[k], B, h, h, POOL_C[k], 0, POOL_C[k], dcat, h, h, cs, 0, FEA, 3, 1, 1, W_of(l), b_of(l), acc, scratch, bp.scratch, stream));
            if (dpool[k]) GEN(vstab_conv_dgrad(dcat, B, h, h, cs, 0, FEA, w + o.raw_w[l], nullptr, 3, 1, 1, dpool[k], h, h, POOL_C[k], 0, POOL_C[k], k == 4 ? 1 : 0, scratch, bp.scratch, stream));
        }
    }
#undef GEN
    return VSTAB_OK;
}

// ---- the walk's own kernels, one stage at a time (tests/test_gpu_nldf_backward.py)
extern "C" size_t vstab_nldf_score_backward_workspace_bytes(int B)
{
    if (B < 1 || B > 64) return 0;
    return score_part_bytes(B) + score_lsw_bytes();
}

extern "C" int vstab_nldf_score_backward(const float *dscore, const float *prob, const float *dprob, const float *local_fea, const float *dlocal_fea,
                                         const float *W, int B, float *dls, float *dgs, float *dlf, float *dW, float *db2, int accumulate,
                                         void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!dscore || !dgs || !workspace) return fail(nullptr, VSTAB_E_STATE, "nldf_score_backward: NULL buffer");
    if (dprob && (!prob || !dls)) return fail(nullptr, VSTAB_E_STATE, "nldf_score_backward: dprob needs prob and dls");
    if ((dlf && !W) || (dW && !local_fea)) return fail(nullptr, VSTAB_E_STATE, "nldf_score_backward: dlf needs W, dW needs local_fea");
    if (B < 1 || B > 64 || (long long)B * NPIX * LF_C * 4 >= 0x80000000LL) return fail(nullptr, VSTAB_E_SHAPE, "nldf_score_backward: unsupported batch %d", B);
    if (((uintptr_t)dscore | (uintptr_t)prob | (uintptr_t)dprob | (uintptr_t)local_fea | (uintptr_t)dlocal_fea | (uintptr_t)W | (uintptr_t)dls |
         (uintptr_t)dgs | (uintptr_t)dlf | (uintptr_t)dW | (uintptr_t)db2) & 7)
        return fail(nullptr, VSTAB_E_ALIGN, "nldf_score_backward: tensors must be 8-byte aligned");
    if (((uintptr_t)local_fea | (uintptr_t)dlocal_fea | (uintptr_t)dlf) & 15) return fail(nullptr, VSTAB_E_ALIGN, "nldf_score_backward: feature tensors must be 16-byte aligned");
    if ((uintptr_t)workspace & 255) return fail(nullptr, VSTAB_E_ALIGN, "nldf_score_backward: workspace must be 256-byte aligned");
    if (workspace_bytes < vstab_nldf_score_backward_workspace_bytes(B)) return fail(nullptr, VSTAB_E_NOMEM, "nldf_score_backward: workspace too small");
    hipStream_t stream = (hipStream_t)stream_;
    float *part = static_cast<float *>(workspace);
    float *slabs = reinterpret_cast<float *>(static_cast<char *>(workspace) + score_part_bytes(B));
    const float *g = dprob ? dls : dscore;
    HIP_TRY(nullptr, launch_nldf_score_grad(dscore, prob, dprob, B, NPIX, dls, part, stream));
    HIP_TRY(nullptr, launch_nldf_score_fold(part, B, nullptr, nullptr, nullptr, dgs, nullptr, nullptr, db2, nullptr, accumulate, stream));
    if (dW) HIP_TRY(nullptr, launch_local_score_wgrad(local_fea, g, (long long)B * NPIX, LF_C, dW, accumulate, slabs, stream));
    if (dlf) HIP_TRY(nullptr, launch_local_score_dgrad(g, W, (long long)B * NPIX, LF_C, dlocal_fea, dlf, stream));
    return VSTAB_OK;
}

extern "C" int vstab_nldf_contrast_gate_backward(const float *act, float *dcat, int B, int H, int W, int C, int cs, void *stream)
{
    if (!act || !dcat) return fail(nullptr, VSTAB_E_STATE, "nldf_contrast_gate_backward: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || (cs & 3) || cs < 2 * C || (long long)B * H * W * cs * 4 >= 0x80000000LL)
        return fail(nullptr, VSTAB_E_SHAPE, "nldf_contrast_gate_backward: bad shape (C, cs multiples of 4, cs >= 2 C)");
    if (((uintptr_t)act | (uintptr_t)dcat) & 15) return fail(nullptr, VSTAB_E_ALIGN, "nldf_contrast_gate_backward: 16-byte tensors");
    HIP_TRY(nullptr, launch_contrast_gate_backward(act, dcat, B, H, W, C, cs, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_nldf_slice_gate_backward(const float *act, float *d, long long rows, int cs, int c_off, int C, float *db, int accumulate,
                                              void *workspace, size_t workspace_bytes, void *stream)
{
    if (!act || !d || (db && !workspace)) return fail(nullptr, VSTAB_E_STATE, "nldf_slice_gate_backward: NULL buffer");
    if (rows < 1 || C < 4 || (C & 3) || (cs & 3) || (c_off & 3) || c_off < 0 || c_off + C > cs || rows * cs * 4 >= 0x80000000LL)
        return fail(nullptr, VSTAB_E_SHAPE, "nldf_slice_gate_backward: bad shape (C, cs, c_off multiples of 4)");
    if (((uintptr_t)act | (uintptr_t)d | (uintptr_t)workspace) & 15) return fail(nullptr, VSTAB_E_ALIGN, "nldf_slice_gate_backward: 16-byte tensors");
    if (db && workspace_bytes < (size_t)column_sum_chunks(rows, C) * C * sizeof(float)) return fail(nullptr, VSTAB_E_NOMEM, "nldf_slice_gate_backward: workspace too small");
    HIP_TRY(nullptr, launch_slice_gate(act, d, rows, cs, c_off, C, (hipStream_t)stream));
    if (db) HIP_TRY(nullptr, launch_column_sum(d, rows, cs, c_off, C, db, accumulate ? 1 : 0, static_cast<float *>(workspace), (hipStream_t)stream));
    return VSTAB_OK;
}
