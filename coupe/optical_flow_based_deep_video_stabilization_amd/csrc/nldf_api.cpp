// C ABI of the NLDF saliency head (NLDF.py:24-134).  The reference never
// instantiates this model (no `NLDF.Model(` call anywhere) and the file is Python-2 only, so this is
// built last and only at the reference's hard-wired geometry: pool1..pool5 of a 352x352 input
// (176, 88, 44, 22, 11), outputs at 176x176 (NLDF.py:58-64, 74).
#include <algorithm>

#include "api_internal.h"
#include "conv_desc.h"
#include "nldf_plan.h"

using namespace vstab;

using namespace nldf;

static vstab_nldf *nldf_of(vstab_ctx *ctx)
{
    if (!ctx->nldf) ctx->nldf = new (std::nothrow) vstab_nldf();
    return static_cast<vstab_nldf *>(ctx->nldf);
}

void vstab_nldf_free(void *p)
{
    vstab_nldf *n = static_cast<vstab_nldf *>(p);
    if (!n) return;
    if (n->w) (void)hipFree(n->w);
    delete n;
}

extern "C" size_t vstab_nldf_workspace_bytes(int B)
{
    NldfPlan pl;
    if (!nldf_plan(B, pl)) { fail(nullptr, VSTAB_E_SHAPE, "nldf: unsupported batch %d", B); return 0; }
    return pl.total;
}

extern "C" int vstab_nldf_workspace_layout(int B, vstab_ws_entry *entries, int max_entries)
{
    NldfPlan pl;
    if (!nldf_plan(B, pl)) return fail(nullptr, VSTAB_E_SHAPE, "nldf: unsupported batch %d", B);
    if (!entries || max_entries < 0) return fail(nullptr, VSTAB_E_STATE, "nldf_workspace_layout: no entries");
    int n = 0;
    for (int i = 0; i < N_NBUF && n < max_entries; ++i, ++n) {
        const NBufSpec &s = NBUFS[i];
        vstab_ws_entry &e = entries[n];
        std::memset(&e, 0, sizeof(e));
        std::strncpy(e.name, s.name, sizeof(e.name) - 1);
        e.offset_bytes = (int64_t)pl.off[i];
        if (s.hw) { e.n = B; e.h = e.w = s.hw; e.c = e.c_stride = s.c; }
        else { e.n = 1; e.h = 0; e.w = 0; e.c = e.c_stride = s.c; }             // h == 0: a flat run of c floats
    }
    return n;
}

extern "C" int vstab_nldf_load(vstab_ctx *ctx, const vstab_tensor *t, int count)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "nldf_load: ctx is NULL");
    if (!t || count <= 0) return fail(ctx, VSTAB_E_WEIGHTS, "nldf_load: no tensors");
    vstab_nldf *N = nldf_of(ctx);
    if (!N) return fail(ctx, VSTAB_E_NOMEM, "nldf_load: out of host memory");
    std::vector<float> host;
    auto reserve = [&](size_t n) { size_t o = (host.size() + 63) / 64 * 64; host.resize(o + n, 0.f); return o; };
    std::vector<double> ones;
    // plain conv: W [k][k][cin][cout], b [cout]
    auto conv = [&](const std::string &name, int k, int cin, int cs_in, int cout, size_t &ow, size_t &ob) -> bool {
        const vstab_tensor *W = find(t, count, name + "/W"), *b = find(t, count, name + "/b");
        if (!shape_is(W, {k, k, cin, cout}) || !shape_is(b, {cout})) { fail(ctx, VSTAB_E_WEIGHTS, "missing or mis-shaped variable %s/{W,b}", name.c_str()); return false; }
        const int npad = padded_cols(cout);
        const KLayout L = conv_layout(k, k, cin, cs_in);
        ones.assign(npad, 1.0);
        ob = reserve(npad);
        fold_bn(b->data, nullptr, nullptr, nullptr, cout, npad, ones.data(), host.data() + ob);
        ow = reserve((size_t)L.ktiles() * npad * 32);
        pack_conv(W->data, ones.data(), k, k, cin, cs_in, cout, npad, L, host.data() + ow);
        return true;
    };
    NldfWeights &o = N->o;
    if (!conv("Fea_Global_1", 5, 512, 512, FEA, o.g1_w, o.g1_b)) return VSTAB_E_WEIGHTS;
    if (!conv("Fea_Global_2", 5, FEA, FEA, FEA, o.g2_w, o.g2_b)) return VSTAB_E_WEIGHTS;
    if (!conv("Fea_Global", 3, FEA, FEA, FEA, o.g3_w, o.g3_b)) return VSTAB_E_WEIGHTS;
    for (int k = 0; k < 5; ++k)
        if (!conv("Fea_P" + std::to_string(k + 1), 3, POOL_C[k], POOL_C[k], FEA, o.p_w[k], o.p_b[k])) return VSTAB_E_WEIGHTS;
    for (int k = 0; k < 4; ++k) {               // Fea_P(k+2)_Deconv: cat(k+2) -> UP_C[k]
        const std::string name = "Fea_P" + std::to_string(k + 2) + "_Deconv";
        const int cin = CAT_C[k + 1], cout = UP_C[k];
        const vstab_tensor *W = find(t, count, name + "/W"), *b = find(t, count, name + "/b");
        if (!shape_is(W, {5, 5, cout, cin}) || !shape_is(b, {cout})) return fail(ctx, VSTAB_E_WEIGHTS, "missing or mis-shaped variable %s/{W,b}", name.c_str());
        const int npad = padded_cols(cout);
        ones.assign(npad, 1.0);
        o.d_b[k] = reserve(npad);
        fold_bn(b->data, nullptr, nullptr, nullptr, cout, npad, ones.data(), host.data() + o.d_b[k]);
        o.d_w[k] = reserve(4 * (size_t)klayout_run(3, 3, cin).ktiles() * npad * 32);
        pack_deconv5(W->data, ones.data(), cin, cin, cout, npad, host.data() + o.d_w[k]);
    }
    if (!conv("Local_Fea", 1, 768, 768, 640, o.lf_w, o.lf_b)) return VSTAB_E_WEIGHTS;
    if (!conv("Local_Score", 1, 640, 640, 2, o.ls_w, o.ls_b)) return VSTAB_E_WEIGHTS;
    if (!conv("Global_Score", 1, FEA, FEA, 2, o.gs_w, o.gs_b)) return VSTAB_E_WEIGHTS;
    // every variable as given, for the backward (nldf_grad_api.cpp): found and shape-checked above
    static const char *const LAYERS[L_COUNT] = {"Fea_Global_1", "Fea_Global_2", "Fea_Global", "Fea_P1", "Fea_P2", "Fea_P3", "Fea_P4", "Fea_P5",
                                                "Fea_P5_Deconv", "Fea_P4_Deconv", "Fea_P3_Deconv", "Fea_P2_Deconv", "Local_Fea", "Local_Score",
                                                "Global_Score"};
    for (int i = 0; i < L_COUNT; ++i) {
        const vstab_tensor *W = find(t, count, std::string(LAYERS[i]) + "/W"), *b = find(t, count, std::string(LAYERS[i]) + "/b");
        const size_t nw = (size_t)W->shape[0] * W->shape[1] * W->shape[2] * W->shape[3], nb = (size_t)b->shape[0];
        o.raw_w[i] = reserve(nw);
        std::copy(W->data, W->data + nw, host.begin() + o.raw_w[i]);
        o.raw_b[i] = reserve(nb);
        std::copy(b->data, b->data + nb, host.begin() + o.raw_b[i]);
    }

    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (N->w) { (void)hipFree(N->w); N->w = nullptr; }
    N->loaded = false;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&N->w), host.size() * sizeof(float));
    if (e != hipSuccess) return fail(ctx, VSTAB_E_NOMEM, "hipMalloc(%zu bytes of NLDF weights): %s", host.size() * 4, hipGetErrorString(e));
    HIP_TRY(ctx, hipMemcpy(N->w, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    N->loaded = true;
    return VSTAB_OK;
}

extern "C" int vstab_nldf_forward(vstab_ctx *ctx, const float *const *pools5, int B, float *prob, float *score, float *local_fea,
                                  float *fea_global, void *workspace, size_t workspace_bytes, void *stream_)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "nldf_forward: ctx is NULL");
    vstab_nldf *N = nldf_of(ctx);
    if (!N || !N->loaded) return fail(ctx, VSTAB_E_STATE, "nldf_forward: vstab_nldf_load has not been called");
    if (!pools5 || !prob || !workspace) return fail(ctx, VSTAB_E_STATE, "nldf_forward: NULL buffer");
    for (int k = 0; k < 5; ++k)
        if (!pools5[k] || ((uintptr_t)pools5[k] & 15)) return fail(ctx, VSTAB_E_ALIGN, "nldf_forward: pool%d NULL or not 16-byte aligned", k + 1);
    NldfPlan pl;
    if (!nldf_plan(B, pl)) return fail(ctx, VSTAB_E_SHAPE, "nldf_forward: unsupported batch %d", B);
    if (workspace_bytes < pl.total) return fail(ctx, VSTAB_E_NOMEM, "nldf_forward: workspace %zu < %zu bytes", workspace_bytes, pl.total);
    if ((uintptr_t)workspace & 255) return fail(ctx, VSTAB_E_ALIGN, "nldf_forward: workspace must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    char *ws = (char *)workspace;
    auto buf = [&](int b) { return (float *)(ws + pl.off[b]); };
    const float *w = N->w;
    const NldfWeights &o = N->o;
    float *part = buf(N_PART);
    const size_t part_floats = pl.bytes[N_PART] / 4;

    auto run_conv = [&](const float *in, int hw_in, int cin, int cs_in, int k, int pad, int cout, float *out, int cs_out, int c_off,
                        int act, size_t ow, size_t ob) -> int {
        ConvParams p; ConvTile tile; bool vec;
        if (!fill_plain_conv(p, tile, vec, B, hw_in, hw_in, cin, cs_in, k, 1, pad, cout, cs_out, c_off, act))
            return fail(ctx, VSTAB_E_SHAPE, "nldf_forward: conv %dx%d on %d does not fit", k, k, hw_in);
        if (p.ksplit > 1 && (size_t)p.ksplit * p.Mmax * p.Npad > part_floats) p.ksplit = 1;
        if (p.ksplit > 1 && ((cout & 3) || (cs_out & 3) || (c_off & 3))) p.ksplit = 1;
        p.in = in; p.out = out; p.wpk = w + ow; p.bias = w + ob; p.partial = part;
        HIP_TRY(ctx, launch_conv(p, tile, vec, stream));
        return VSTAB_OK;
    };
#define RUN(...) do { const int rc_ = run_conv(__VA_ARGS__); if (rc_ != VSTAB_OK) return rc_; } while (0)

    // global branch (NLDF.py:36-41): 5x5 VALID, 5x5 VALID (ReLU), 3x3 VALID (linear) on pool5: 11 -> 7 -> 3 -> 1
    RUN(pools5[4], 11, 512, 512, 5, 0, FEA, buf(N_G1), FEA, 0, 2, o.g1_w, o.g1_b);
    RUN(buf(N_G1), 7, FEA, FEA, 5, 0, FEA, buf(N_G2), FEA, 0, 2, o.g2_w, o.g2_b);
    RUN(buf(N_G2), 3, FEA, FEA, 3, 0, FEA, buf(N_G), FEA, 0, 0, o.g3_w, o.g3_b);
    // local features (:44-48) + contrast (:50-54) into the first 256 channels of cat1..cat5
    const int cat_buf[5] = {N_CAT1, N_CAT2, N_CAT3, N_CAT4, N_CAT5};
    for (int k = 0; k < 5; ++k) {
        RUN(pools5[k], POOL_HW[k], POOL_C[k], POOL_C[k], 3, 1, FEA, buf(cat_buf[k]), CAT_C[k], 0, 2, o.p_w[k], o.p_b[k]);
        HIP_TRY(ctx, launch_contrast(buf(cat_buf[k]), B, POOL_HW[k], POOL_HW[k], FEA, CAT_C[k], FEA, stream));
    }
    // top-down 5x5 stride-2 transposed convs + ReLU (:57-64): cat5 -> cat4[256:], ..., cat2 -> cat1[256:]
    for (int k = 3; k >= 0; --k) {
        const int hin = POOL_HW[k + 1], hout = POOL_HW[k], cin = CAT_C[k + 1], cout = UP_C[k];
        const int off[2] = {-1, -1};             // 3 taps from input row j - 1 in both parities (the even ones use two: pack_deconv5)
        ConvParams p = conv_desc_parity4(B, hin, hin, cin, cin, 3, off, hout, hout, cout, padded_cols(cout), CAT_C[k], 2 * FEA, 2);
        choose_split(p, 128);
        if ((size_t)p.nphase * p.ksplit * p.Mmax * p.Npad > part_floats) p.ksplit = 1;
        p.in = buf(cat_buf[k + 1]); p.out = buf(cat_buf[k]); p.wpk = w + o.d_w[k]; p.bias = w + o.d_b[k]; p.partial = part;
        HIP_TRY(ctx, launch_conv(p, TILE_128x128, true, stream));
    }
    // scores (:66-77)
    float *lf = local_fea ? local_fea : buf(N_LF);
    RUN(buf(N_CAT1), 176, 768, 768, 1, 0, 640, lf, 640, 0, 0, o.lf_w, o.lf_b);
    RUN(lf, 176, 640, 640, 1, 0, 2, buf(N_LS), 2, 0, 0, o.ls_w, o.ls_b);
    RUN(buf(N_G), 1, FEA, FEA, 1, 0, 2, buf(N_GS), 2, 0, 0, o.gs_w, o.gs_b);
#undef RUN
    HIP_TRY(ctx, launch_nldf_score(buf(N_LS), buf(N_GS), B, 176 * 176, score, prob, stream));
    if (fea_global)
        HIP_TRY(ctx, hipMemcpyAsync(fea_global, buf(N_G), sizeof(float) * (size_t)B * FEA, hipMemcpyDeviceToDevice, stream));
    return VSTAB_OK;
}
