// C ABI of the VGG16 trunk (vgg16.py): thirteen 3x3 convolutions + ReLU and five 2x2 max pools, every activation returned.
#include "api_internal.h"
#include "conv_desc.h"
#include "vgg_plan.h"

using namespace vstab;

const VggLayer VGG[13] = {{"conv1_1", 3, 64, false},   {"conv1_2", 64, 64, true},    {"conv2_1", 64, 128, false},
                          {"conv2_2", 128, 128, true}, {"conv3_1", 128, 256, false}, {"conv3_2", 256, 256, false},
                          {"conv3_3", 256, 256, true}, {"conv4_1", 256, 512, false}, {"conv4_2", 512, 512, false},
                          {"conv4_3", 512, 512, true}, {"conv5_1", 512, 512, false}, {"conv5_2", 512, 512, false},
                          {"conv5_3", 512, 512, true}};

bool vgg_plan(int B, int H, int W, VggPlan &v)
{
    if (B < 1 || H < 1 || W < 1) return false;
    int h = H, w = W, o = 0;
    v.partial_floats = v.wino_v = v.wino_m = 0;
    for (int l = 0; l < 13; ++l) {
        ConvParams p; ConvTile t; bool vec;
        if (!fill_plain_conv(p, t, vec, B, h, w, VGG[l].cin, VGG[l].cin, 3, 1, 1, VGG[l].cout, VGG[l].cout, 0, 2)) return false;
        v.wino[l] = VGG[l].cin >= 256 && wino_applies(B, h, w, VGG[l].cin, VGG[l].cout);     // conv3_2 .. conv5_3 when the level is large enough
        if (v.wino[l]) {
            const size_t tiles = (size_t)B * 16 * ((h + 1) / 2) * ((w + 1) / 2);
            v.wino_v = std::max(v.wino_v, tiles * VGG[l].cin);
            v.wino_m = std::max(v.wino_m, tiles * VGG[l].cout);
        } else if (p.ksplit > 1) v.partial_floats = std::max(v.partial_floats, (size_t)p.ksplit * p.Mmax * p.Npad);
        v.h[o] = h; v.w[o] = w; v.c[o] = VGG[l].cout; ++o;
        if (VGG[l].pool_after) {
            h = (h + 1) / 2; w = (w + 1) / 2;
            v.h[o] = h; v.w[o] = w; v.c[o] = VGG[l].cout; ++o;
        }
    }
    return true;
}

namespace {
size_t vgg_ws_bytes(const VggPlan &v)       // [split-K slabs | Winograd V | Winograd M], each 256-byte aligned
{
    return a256(std::max<size_t>(v.partial_floats * 4, 256)) + a256(v.wino_v * 4) + a256(v.wino_m * 4);
}

}  // namespace

int vgg_max_chunk(int B, int H, int W)
{
    VggPlan v;
    return largest_fitting(B, [&](int b) { return vgg_plan(b, H, W, v); });
}

extern "C" int vstab_vgg16_shapes(int H, int W, int32_t *hwc54)
{
    VggPlan v;
    if (!hwc54 || !vgg_plan(1, H, W, v)) return fail(nullptr, VSTAB_E_SHAPE, "vgg16: unsupported input %dx%d", H, W);
    for (int i = 0; i < 18; ++i) { hwc54[3 * i] = v.h[i]; hwc54[3 * i + 1] = v.w[i]; hwc54[3 * i + 2] = v.c[i]; }
    return VSTAB_OK;
}

extern "C" size_t vstab_vgg16_workspace_bytes(int B, int H, int W)
{
    const int chunk = B >= 1 ? vgg_max_chunk(B, H, W) : 0;
    VggPlan v;
    if (chunk < 1 || !vgg_plan(chunk, H, W, v)) { fail(nullptr, VSTAB_E_SHAPE, "vgg16: unsupported problem %dx%dx%d", B, H, W); return 0; }
    return vgg_ws_bytes(v);
}

extern "C" int vstab_vgg16_load(vstab_ctx *ctx, const vstab_tensor *t, int count)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "vgg16_load: ctx is NULL");
    if (!t || count <= 0) return fail(ctx, VSTAB_E_WEIGHTS, "vgg16_load: no tensors");
    std::vector<float> host;
    auto reserve = [&](size_t n) { size_t o = (host.size() + 63) / 64 * 64; host.resize(o + n, 0.f); return o; };
    std::vector<double> ones;
    ctx->vgg_zero = reserve(1024);              // zero bias for the Winograd-domain GEMMs (the inverse transform adds the real one)
    for (int l = 0; l < 13; ++l) {
        const std::string n = VGG[l].name;
        const vstab_tensor *W = find(t, count, n + "/filter"), *b = find(t, count, n + "/biases");
        if (!shape_is(W, {3, 3, VGG[l].cin, VGG[l].cout}) || !shape_is(b, {VGG[l].cout}))
            return fail(ctx, VSTAB_E_WEIGHTS, "missing or mis-shaped variable %s/{filter,biases}", n.c_str());
        const int npad = padded_cols(VGG[l].cout);
        const KLayout L = klayout_run(3, 3, VGG[l].cin);
        ones.assign(npad, 1.0);
        ctx->vgg_b[l] = reserve(npad);
        fold_bn(b->data, nullptr, nullptr, nullptr, VGG[l].cout, npad, ones.data(), host.data() + ctx->vgg_b[l]);
        ctx->vgg_w[l] = reserve((size_t)L.ktiles() * npad * 32);
        pack_conv(W->data, ones.data(), 3, 3, VGG[l].cin, VGG[l].cin, VGG[l].cout, npad, L, host.data() + ctx->vgg_w[l]);
        // the filter as given (HWIO): conv1_1's store-shaped kernel reads it, and so do the backward's launchers (vgg_grad_api.cpp)
        ctx->vgg_raw[l] = reserve((size_t)9 * VGG[l].cin * VGG[l].cout);
        std::memcpy(host.data() + ctx->vgg_raw[l], W->data, sizeof(float) * 9 * VGG[l].cin * VGG[l].cout);
        if (l == 0) ctx->vgg_raw0 = ctx->vgg_raw[0];
        ctx->vgg_wino_w[l] = 0;
        if (VGG[l].cin >= 256) {                       // Winograd-domain operand for the layers that may run in that form
            ctx->vgg_wino_w[l] = reserve((size_t)16 * (VGG[l].cin / 32) * VGG[l].cout * 32);
            pack_winograd(W->data, ones.data(), VGG[l].cin, VGG[l].cout, VGG[l].cout, host.data() + ctx->vgg_wino_w[l]);
        }
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (ctx->vgg_weights) { (void)hipFree(ctx->vgg_weights); ctx->vgg_weights = nullptr; }
    ctx->vgg_loaded = false;
    vgg_backward_free(ctx);                        // operands derived from the previous filters
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&ctx->vgg_weights), host.size() * sizeof(float));
    if (e != hipSuccess) return fail(ctx, VSTAB_E_NOMEM, "hipMalloc(%zu bytes of VGG16 weights): %s", host.size() * 4, hipGetErrorString(e));
    HIP_TRY(ctx, hipMemcpy(ctx->vgg_weights, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    ctx->vgg_loaded = true;
    return VSTAB_OK;
}

extern "C" int vstab_vgg16_forward(vstab_ctx *ctx, const float *input, int B, int H, int W, float *const *outs, void *workspace,
                                   size_t workspace_bytes, void *stream_)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "vgg16_forward: ctx is NULL");
    if (!ctx->vgg_loaded) return fail(ctx, VSTAB_E_STATE, "vgg16_forward: vstab_vgg16_load has not been called");
    if (!input || !outs || !workspace) return fail(ctx, VSTAB_E_STATE, "vgg16_forward: NULL buffer");
    for (int i = 0; i < 18; ++i)
        if (!outs[i] || ((uintptr_t)outs[i] & 15)) return fail(ctx, VSTAB_E_ALIGN, "vgg16_forward: output %d NULL or not 16-byte aligned", i);
    const int cmax = B >= 1 ? vgg_max_chunk(B, H, W) : 0;
    if (cmax < 1) return fail(ctx, VSTAB_E_SHAPE, "vgg16_forward: unsupported problem %dx%dx%d", B, H, W);
    const int nchunks = (B + cmax - 1) / cmax, chunk = (B + nchunks - 1) / nchunks;
    VggPlan v;
    if (!vgg_plan(chunk, H, W, v)) return fail(ctx, VSTAB_E_SHAPE, "vgg16_forward: plan failed");
    if (workspace_bytes < vgg_ws_bytes(v)) return fail(ctx, VSTAB_E_NOMEM, "vgg16_forward: workspace %zu < %zu bytes", workspace_bytes, vgg_ws_bytes(v));
    if ((uintptr_t)workspace & 255) return fail(ctx, VSTAB_E_ALIGN, "vgg16_forward: workspace must be 256-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    float *wsV = reinterpret_cast<float *>(static_cast<char *>(workspace) + a256(std::max<size_t>(v.partial_floats * 4, 256)));
    float *wsM = reinterpret_cast<float *>(reinterpret_cast<char *>(wsV) + a256(v.wino_v * 4));
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int bc = std::min(chunk, B - b0);
        const float *cur = input + (size_t)b0 * H * W * 3;
        int h = H, w = W, o = 0;
        for (int l = 0; l < 13; ++l) {
            ConvParams p; ConvTile tile; bool vec;
            if (!fill_plain_conv(p, tile, vec, bc, h, w, VGG[l].cin, VGG[l].cin, 3, 1, 1, VGG[l].cout, VGG[l].cout, 0, 2))
                return fail(ctx, VSTAB_E_SHAPE, "vgg16_forward: layer %s does not fit", VGG[l].name);
            float *dst = outs[o] + (size_t)b0 * v.h[o] * v.w[o] * v.c[o];
            if (l == 0) {
                HIP_TRY(ctx, launch_conv3x3_rgb(cur, bc, h, w, ctx->vgg_weights + ctx->vgg_raw0, ctx->vgg_weights + ctx->vgg_b[0], VGG[0].cout, 1, dst, stream));
            } else if (v.wino[l] && wino_applies(bc, h, w, VGG[l].cin, VGG[l].cout)) {      // (a short last chunk may fall below the break-even)
                ConvParams q = conv_desc_wino_gemm(bc, h, w, VGG[l].cin, VGG[l].cout);
                HIP_TRY(ctx, launch_wino_input(cur, bc, h, w, VGG[l].cin, 0, VGG[l].cin, wsV, stream));
                q.in = wsV; q.out = wsM; q.wpk = ctx->vgg_weights + ctx->vgg_wino_w[l]; q.bias = ctx->vgg_weights + ctx->vgg_zero;
                HIP_TRY(ctx, launch_conv(q, TILE_128x64, true, stream));
                HIP_TRY(ctx, launch_wino_output(wsM, bc, h, w, VGG[l].cout, ctx->vgg_weights + ctx->vgg_b[l], 2, dst, VGG[l].cout, 0, stream));
            } else {
                p.in = cur; p.out = dst; p.wpk = ctx->vgg_weights + ctx->vgg_w[l]; p.bias = ctx->vgg_weights + ctx->vgg_b[l];
                p.partial = (float *)workspace;
                HIP_TRY(ctx, launch_conv(p, tile, vec, stream));
            }
            cur = dst; ++o;
            if (VGG[l].pool_after) {
                float *pd = outs[o] + (size_t)b0 * v.h[o] * v.w[o] * v.c[o];
                HIP_TRY(ctx, launch_maxpool2x2(cur, bc, h, w, VGG[l].cout, pd, stream));
                h = (h + 1) / 2; w = (w + 1) / 2;
                cur = pd; ++o;
            }
        }
    }
    return VSTAB_OK;
}
