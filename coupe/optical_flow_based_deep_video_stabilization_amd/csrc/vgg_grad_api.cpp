// C ABI of the VGG16 trunk's backward (vgg16.py: Vgg16.backward / features): the reverse walk over the 13
// convolutions and 5 pools with gradients entering at any of the 18 outputs, and thin entries to its three own kernels.  No
// arithmetic here: the gates and the first layer are vgg_grad_ops.hip, every other convolution gradient goes through the training
// convolutions' entry points (train_conv_api.cpp) or the forward's Winograd launchers on a transposed operand.
#include <algorithm>

#include "api_internal.h"
#include "conv_desc.h"
#include "vgg_plan.h"

using namespace vstab;

namespace {
// output index of layer l's convolution in build() order (its pool, if any, is the next one)
int conv_out_index(int l)
{
    int o = 0;
    for (int i = 0; i < l; ++i) o += VGG[i].pool_after ? 2 : 1;
    return o;
}

// does layer l's input gradient run in the transposed Winograd form?  The forward's rule with the channel roles swapped.
bool dgrad_wino(int l, int bc, int h, int w) { return l > 0 && VGG[l].cin >= 256 && wino_applies(bc, h, w, VGG[l].cout, VGG[l].cin); }

// Workspace: [gradient buffer 0 | gradient buffer 1 | scratch of the layer at work], each 256-byte aligned.  A gradient buffer holds
// the largest activation of one chunk; the scratch is the largest any launch of any layer asks for, at both chunk sizes the batch
// splits into.
struct BwdWs { size_t buf, scratch, total; };

size_t layer_scratch(int l, int bc, int h, int w, bool need_weights)
{
    const int ci = VGG[l].cin, co = VGG[l].cout;
    size_t s = 0;
    if (l == 0) return need_weights ? conv3x3_rgb_wgrad_scratch_bytes((long long)bc * h * w) : 0;
    if (dgrad_wino(l, bc, h, w)) {
        const size_t tiles = (size_t)bc * 16 * ((h + 1) / 2) * ((w + 1) / 2);
        s = std::max(a256(tiles * co * 4) + a256(tiles * ci * 4), a256((size_t)16 * ci * co * 4));      // V | M, or the filter transform while it is packed
    } else {
        s = vstab_conv_dgrad_workspace_bytes(bc, h, w, co, co, 3, 1, 1, h, w, ci, 0, ci, 0);
        if (s == 0) return (size_t)-1;
    }
    if (need_weights) s = std::max(s, vstab_conv_wgrad_workspace_bytes(bc, h, w, 3, ci, co));
    return s;
}

bool bwd_ws(int B, int H, int W, bool need_weights, int &chunk, VggPlan &v, BwdWs &ws)
{
    const int cmax = B >= 1 ? vgg_max_chunk(B, H, W) : 0;
    if (cmax < 1) return false;
    const int nchunks = (B + cmax - 1) / cmax;
    chunk = (B + nchunks - 1) / nchunks;
    if (!vgg_plan(chunk, H, W, v)) return false;
    size_t act = 0;
    for (int i = 0; i < 18; ++i) act = std::max(act, (size_t)chunk * v.h[i] * v.w[i] * v.c[i]);
    ws.buf = a256(act * sizeof(float));
    ws.scratch = 256;
    const int tail = B - (nchunks - 1) * chunk;
    for (int bc : {chunk, tail}) {
        if (bc < 1) continue;
        for (int l = 0; l < 13; ++l) {
            const int o = conv_out_index(l);
            const size_t s = layer_scratch(l, bc, v.h[o], v.w[o], need_weights);
            if (s == (size_t)-1) return false;
            ws.scratch = std::max(ws.scratch, a256(s));
        }
    }
    ws.total = 2 * ws.buf + ws.scratch;
    return true;
}
}  // namespace

void vgg_backward_free(vstab_ctx *ctx)
{
    for (int l = 0; l < 13; ++l)
        if (ctx->vgg_bwd_wino[l]) { (void)hipFree(ctx->vgg_bwd_wino[l]); ctx->vgg_bwd_wino[l] = nullptr; }
}

extern "C" size_t vstab_vgg16_backward_workspace_bytes(int B, int H, int W, int need_weights)
{
    int chunk; VggPlan v; BwdWs ws;
    if (!bwd_ws(B, H, W, need_weights != 0, chunk, v, ws)) { fail(nullptr, VSTAB_E_SHAPE, "vgg16_backward: unsupported problem %dx%dx%d", B, H, W); return 0; }
    return ws.total;
}

extern "C" int vstab_vgg16_backward(vstab_ctx *ctx, const float *input, int B, int H, int W, float *const *outs, const float *const *douts,
                                    float *dinput, float *const *dparams, int accumulate_params, void *workspace, size_t workspace_bytes,
                                    void *stream_)
{
    if (!ctx) return fail(nullptr, VSTAB_E_STATE, "vgg16_backward: ctx is NULL");
    if (!ctx->vgg_loaded) return fail(ctx, VSTAB_E_STATE, "vgg16_backward: vstab_vgg16_load has not been called");
    if (!input || !outs || !douts || !workspace) return fail(ctx, VSTAB_E_STATE, "vgg16_backward: NULL buffer");
    if (!dinput && !dparams) return fail(ctx, VSTAB_E_STATE, "vgg16_backward: neither the input gradient nor the filter gradients are asked for");
    int top = -1;
    for (int i = 0; i < 18; ++i) {
        if (!outs[i]) return fail(ctx, VSTAB_E_STATE, "vgg16_backward: output %d is NULL", i);
        if (douts[i]) top = i;
    }
    if (top < 0) return fail(ctx, VSTAB_E_STATE, "vgg16_backward: no output carries a gradient");
    for (int i = 0; i < 18; ++i)
        if (((uintptr_t)outs[i] & 15) || ((uintptr_t)douts[i] & 15)) return fail(ctx, VSTAB_E_ALIGN, "vgg16_backward: output %d or its gradient is not 16-byte aligned", i);
    if (((uintptr_t)input & 15) || ((uintptr_t)dinput & 15)) return fail(ctx, VSTAB_E_ALIGN, "vgg16_backward: input / dinput must be 16-byte aligned");
    if (dparams)
        for (int i = 0; i < 26; ++i)
            if ((uintptr_t)dparams[i] & 15) return fail(ctx, VSTAB_E_ALIGN, "vgg16_backward: parameter gradient %d is not 16-byte aligned", i);
    if ((uintptr_t)workspace & 255) return fail(ctx, VSTAB_E_ALIGN, "vgg16_backward: workspace must be 256-byte aligned");
    bool any_param = false;
    if (dparams) for (int i = 0; i < 26; ++i) any_param = any_param || dparams[i];
    if (!dinput && !any_param) return fail(ctx, VSTAB_E_STATE, "vgg16_backward: neither the input gradient nor a filter gradient is asked for");
    int chunk; VggPlan v; BwdWs ws;
    if (!bwd_ws(B, H, W, any_param, chunk, v, ws)) return fail(ctx, VSTAB_E_SHAPE, "vgg16_backward: unsupported problem %dx%dx%d", B, H, W);
    if (workspace_bytes < ws.total) return fail(ctx, VSTAB_E_NOMEM, "vgg16_backward: workspace %zu < %zu bytes", workspace_bytes, ws.total);

    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, conv_set_attributes());
    char *wsb = static_cast<char *>(workspace);
    float *bufs[2] = {reinterpret_cast<float *>(wsb), reinterpret_cast<float *>(wsb + ws.buf)};
    void *scratch = wsb + 2 * ws.buf;
    auto other = [&](const float *p) { return p == bufs[0] ? bufs[1] : bufs[0]; };
    auto wants = [&](int l) { return dparams && (dparams[2 * l] || dparams[2 * l + 1]); };
    const bool need0 = dinput || wants(0);                      // does anything ask for work at conv1_1?
    int lmax = 12;
    while (conv_out_index(lmax) > top) --lmax;                  // layers above the deepest gradient are never touched
    const float *zeros = ctx->vgg_weights + ctx->vgg_zero;

    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int bc = std::min(chunk, B - b0);
        const int acc_p = (accumulate_params || b0 > 0) ? 1 : 0;        // filter gradients accumulate across chunks
        auto out_at = [&](int i) { return outs[i] + (size_t)b0 * v.h[i] * v.w[i] * v.c[i]; };
        auto dout_at = [&](int i) { return douts[i] ? douts[i] + (size_t)b0 * v.h[i] * v.w[i] * v.c[i] : nullptr; };
        float *run = nullptr;                                   // running gradient at the output of layer l's block (one of bufs)
        for (int l = lmax; l >= (need0 ? 0 : 1); --l) {
            const int oc = conv_out_index(l), op = oc + 1, ci = VGG[l].cin, co = VGG[l].cout, h = v.h[oc], w = v.w[oc];
            const long long n = (long long)bc * h * w * co;
            const float *y = out_at(oc);
            float *gz;                                          // gradient at this convolution's pre-activation
            if (VGG[l].pool_after && op <= top) {
                const float *gp = run;
                if (run && dout_at(op)) HIP_TRY(ctx, launch_axpby(run, 1.f, dout_at(op), 1.f, run, (long long)bc * v.h[op] * v.w[op] * co, stream));
                else if (!run) gp = dout_at(op);
                gz = run ? other(run) : bufs[0];
                if (dout_at(oc)) HIP_TRY(ctx, hipMemcpyAsync(gz, dout_at(oc), (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, stream));
                HIP_TRY(ctx, launch_maxpool2x2_relu_backward(y, bc, h, w, co, gp, gz, dout_at(oc) ? 1 : 0, stream));
            } else {
                if (run) {
                    gz = run;
                    if (dout_at(oc)) HIP_TRY(ctx, launch_axpby(gz, 1.f, dout_at(oc), 1.f, gz, n, stream));
                } else {
                    gz = bufs[0];                               // l == lmax and the deepest gradient sits at this conv output
                    HIP_TRY(ctx, hipMemcpyAsync(gz, dout_at(oc), (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, stream));
                }
                HIP_TRY(ctx, launch_relu_backward(y, gz, n / 4, stream));
            }
            const float *x = l == 0 ? input + (size_t)b0 * H * W * 3 : out_at(oc - 1);
            const float *Wraw = ctx->vgg_weights + ctx->vgg_raw[l];
            if (wants(l)) {
                if (!dparams[2 * l]) return fail(ctx, VSTAB_E_STATE, "vgg16_backward: %s: a bias gradient without its filter gradient", VGG[l].name);
                if (l == 0) {
                    HIP_TRY(ctx, launch_conv3x3_rgb_wgrad(x, gz, bc, h, w, co, dparams[0], dparams[1], acc_p, static_cast<float *>(scratch), stream));
                } else if (const int c = vstab_conv_wgrad(x, bc, h, w, ci, 0, ci, gz, h, w, co, 0, co, 3, 1, 1, dparams[2 * l], dparams[2 * l + 1], acc_p,
                                                          scratch, ws.scratch, stream)) {
                    adopt_last_error(ctx);
                    return c;
                }
            }
            if (l == 0) {
                if (dinput) HIP_TRY(ctx, launch_conv3x3_rgb_dgrad(gz, bc, h, w, Wraw, co, dinput + (size_t)b0 * H * W * 3, stream));
                break;
            }
            if (l == 1 && !need0) break;
            float *dx = other(gz);
            if (dgrad_wino(l, bc, h, w)) {
                // K = cout reduction channels, N = cin output channels; the operand is transformed and packed once per load
                if (!ctx->vgg_bwd_wino[l]) {
                    float *wpk = nullptr;
                    const hipError_t e = hipMalloc(reinterpret_cast<void **>(&wpk), (size_t)16 * ci * co * sizeof(float));
                    if (e != hipSuccess) return fail(ctx, VSTAB_E_NOMEM, "vgg16_backward: hipMalloc of %s's transposed operand: %s", VGG[l].name, hipGetErrorString(e));
                    hipError_t e2 = launch_wino_weights(Wraw, ci, co, 1, static_cast<float *>(scratch), stream);
                    if (e2 == hipSuccess) e2 = launch_pack_blocked(static_cast<float *>(scratch), co, ci, ci, 16, wpk, stream);
                    if (e2 != hipSuccess) { (void)hipFree(wpk); return fail(ctx, VSTAB_E_HIP, "vgg16_backward: packing %s: %s", VGG[l].name, hipGetErrorString(e2)); }
                    ctx->vgg_bwd_wino[l] = wpk;
                }
                const size_t tiles = (size_t)bc * 16 * ((h + 1) / 2) * ((w + 1) / 2);
                float *V = static_cast<float *>(scratch), *M = reinterpret_cast<float *>(static_cast<char *>(scratch) + a256(tiles * co * 4));
                ConvParams q = conv_desc_wino_gemm(bc, h, w, co, ci);
                HIP_TRY(ctx, launch_wino_input(gz, bc, h, w, co, 0, co, V, stream));
                q.in = V; q.out = M; q.wpk = ctx->vgg_bwd_wino[l]; q.bias = zeros; q.partial = nullptr;
                HIP_TRY(ctx, launch_conv(q, TILE_128x64, true, stream));
                HIP_TRY(ctx, launch_wino_output(M, bc, h, w, ci, zeros, 0, dx, ci, 0, stream));
            } else if (const int c = vstab_conv_dgrad(gz, bc, h, w, co, 0, co, Wraw, nullptr, 3, 1, 1, dx, h, w, ci, 0, ci, 0, scratch, ws.scratch, stream)) {
                adopt_last_error(ctx);
                return c;
            }
            run = dx;
        }
    }
    return VSTAB_OK;
}

// ---- the walk's own kernels, one at a time (tests/test_gpu_vgg_backward.py)
extern "C" int vstab_maxpool2x2_relu_backward(const float *y, int B, int H, int W, int C, const float *dpool, float *dy, int accumulate,
                                              void *stream)
{
    if (!y || !dpool || !dy) return fail(nullptr, VSTAB_E_STATE, "maxpool2x2_relu_backward: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return fail(nullptr, VSTAB_E_SHAPE, "maxpool2x2_relu_backward: bad shape (C must be a multiple of 4)");
    if (((uintptr_t)y | (uintptr_t)dpool | (uintptr_t)dy) & 15) return fail(nullptr, VSTAB_E_ALIGN, "maxpool2x2_relu_backward: 16-byte tensors");
    HIP_TRY(nullptr, launch_maxpool2x2_relu_backward(y, B, H, W, C, dpool, dy, accumulate, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_relu_backward(const float *y, float *dy, long long n, void *stream)
{
    if (!y || !dy) return fail(nullptr, VSTAB_E_STATE, "relu_backward: NULL buffer");
    if (n < 4 || (n & 3)) return fail(nullptr, VSTAB_E_SHAPE, "relu_backward: n must be a positive multiple of 4");
    if (((uintptr_t)y | (uintptr_t)dy) & 15) return fail(nullptr, VSTAB_E_ALIGN, "relu_backward: 16-byte tensors");
    HIP_TRY(nullptr, launch_relu_backward(y, dy, n / 4, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_conv3x3_rgb_dgrad(const float *gout, int B, int H, int W, const float *Wf, int cout, float *dx, void *stream)
{
    if (!gout || !Wf || !dx) return fail(nullptr, VSTAB_E_STATE, "conv3x3_rgb_dgrad: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || cout < 4 || cout > 64 || (cout & 3))
        return fail(nullptr, VSTAB_E_SHAPE, "conv3x3_rgb_dgrad: bad shape (cout a multiple of 4, at most 64)");
    if (((uintptr_t)gout | (uintptr_t)Wf) & 15) return fail(nullptr, VSTAB_E_ALIGN, "conv3x3_rgb_dgrad: gout and W must be 16-byte aligned");
    HIP_TRY(nullptr, launch_conv3x3_rgb_dgrad(gout, B, H, W, Wf, cout, dx, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_conv3x3_rgb_wgrad_workspace_bytes(int B, int H, int W)
{
    if (B < 1 || H < 1 || W < 1) return 0;
    return conv3x3_rgb_wgrad_scratch_bytes((long long)B * H * W);
}

extern "C" int vstab_conv3x3_rgb_wgrad(const float *x, const float *gout, int B, int H, int W, int cout, float *dW, float *db, int accumulate,
                                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (!x || !gout || !dW || !workspace) return fail(nullptr, VSTAB_E_STATE, "conv3x3_rgb_wgrad: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || cout < 4 || cout > 64 || (cout & 3))
        return fail(nullptr, VSTAB_E_SHAPE, "conv3x3_rgb_wgrad: bad shape (cout a multiple of 4, at most 64)");
    if (((uintptr_t)gout | (uintptr_t)workspace) & 15) return fail(nullptr, VSTAB_E_ALIGN, "conv3x3_rgb_wgrad: gout and workspace must be 16-byte aligned");
    if (workspace_bytes < conv3x3_rgb_wgrad_scratch_bytes((long long)B * H * W)) return fail(nullptr, VSTAB_E_NOMEM, "conv3x3_rgb_wgrad: workspace too small");
    HIP_TRY(nullptr, launch_conv3x3_rgb_wgrad(x, gout, B, H, W, cout, dW, db, accumulate, static_cast<float *>(workspace), (hipStream_t)stream));
    return VSTAB_OK;
}
