// C ABI of libvstab_hip.so (include/vstab.h): context, errors, roctx ranges and the thin wrappers around single launches (glue, flow
// warps and their backward, clip-driver pieces, post-filters).  The FlowNetS pyramid lives in flownet_plan.cpp / flownet_forward.cpp,
// the VGG16 trunk in vgg_api.cpp, the NLDF head in nldf_api.cpp, the training blocks in loss_api.cpp, train_conv_api.cpp and train_api.cpp, the samplers in sampler_api.cpp.
#include <cstdlib>
#include <new>

#include "api_internal.h"
#include "vgg_plan.h"

using namespace vstab;

// ------------------------------------------------------------------------- errors
static thread_local std::string g_last_error;

int fail(vstab_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (ctx) { std::lock_guard<std::mutex> g(ctx->err_mu); ctx->err = buf; }
    return code;
}

void adopt_last_error(vstab_ctx *ctx)
{
    if (ctx) { std::lock_guard<std::mutex> g(ctx->err_mu); ctx->err = g_last_error; }
}

// ------------------------------------------------------------------------- roctx ranges
#include <dlfcn.h>
namespace {
typedef int (*roctx_push_t)(const char *);
typedef int (*roctx_pop_t)();
roctx_push_t g_roctx_push = nullptr;
roctx_pop_t g_roctx_pop = nullptr;
bool g_trace_on = false;
}

bool trace_ranges_enable(bool on)
{
    if (on && !g_roctx_push) {
        for (const char *name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            void *h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            g_roctx_push = (roctx_push_t)dlsym(h, "roctxRangePushA");
            g_roctx_pop = (roctx_pop_t)dlsym(h, "roctxRangePop");
            if (g_roctx_push && g_roctx_pop) break;
            g_roctx_push = nullptr; g_roctx_pop = nullptr;
        }
    }
    g_trace_on = on && g_roctx_push != nullptr;
    return !on || g_trace_on;
}

TraceRange::TraceRange(const char *name) : active(g_trace_on)
{
    if (active) g_roctx_push(name);
}
TraceRange::~TraceRange()
{
    if (active) g_roctx_pop();
}

extern "C" int vstab_trace_ranges(int on)
{
    if (!trace_ranges_enable(on != 0)) return fail(nullptr, VSTAB_E_STATE, "trace_ranges: no roctx library (librocprofiler-sdk-roctx.so / libroctx64.so) could be loaded");
    return VSTAB_OK;
}

const vstab_tensor *find(const vstab_tensor *t, int n, const std::string &name)
{
    for (int i = 0; i < n; ++i)
        if (t[i].name && name == t[i].name) return &t[i];
    return nullptr;
}

bool shape_is(const vstab_tensor *t, std::initializer_list<int> s)
{
    if (!t || t->ndim != (int)s.size()) return false;
    int i = 0;
    for (int v : s)
        if (t->shape[i++] != v) return false;
    return t->data != nullptr;
}

// ------------------------------------------------------------------------- context
extern "C" const char *vstab_version(void) { return "vstab-hip 0.1 (gfx950)"; }

extern "C" const char *vstab_last_error(const vstab_ctx *ctx) { return ctx ? ctx->err.c_str() : g_last_error.c_str(); }

extern "C" int vstab_create(vstab_ctx **out, int device)
{
    if (!out) return fail(nullptr, VSTAB_E_STATE, "vstab_create: out is NULL");
    *out = nullptr;
    int n = 0;
    HIP_TRY(nullptr, hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(nullptr, VSTAB_E_HIP, "vstab_create: device %d of %d", device, n);
    HIP_TRY(nullptr, hipSetDevice(device));
    HIP_TRY(nullptr, conv_set_attributes());
    HIP_TRY(nullptr, rowwin_set_attributes());
    HIP_TRY(nullptr, conv1_bf16x3_set_attributes());
    HIP_TRY(nullptr, tap_panel_set_attributes());
    HIP_TRY(nullptr, wino_gemm_stream_set_attributes());
    vstab_ctx *c = new (std::nothrow) vstab_ctx();
    if (!c) return fail(nullptr, VSTAB_E_NOMEM, "vstab_create: out of host memory");
    c->device = device;
    *out = c;
    return VSTAB_OK;
}

extern "C" void vstab_destroy(vstab_ctx *ctx)
{
    if (!ctx) return;
    if (ctx->dev_weights) (void)hipFree(ctx->dev_weights);
    for (hipEvent_t e : ctx->prof_ev) (void)hipEventDestroy(e);
    if (ctx->vgg_weights) (void)hipFree(ctx->vgg_weights);
    vgg_backward_free(ctx);
    vstab_nldf_free(ctx->nldf);
    delete ctx;
}

extern "C" int vstab_host_xcd_remap(int gx, int gy, int gz, int lin, int32_t *xyz)
{
    if (!xyz || gx < 1 || gy < 1 || gz < 1 || lin < 0 || (long long)gx * gy * gz > 0x7fffffffLL || lin >= gx * gy * gz)
        return fail(nullptr, VSTAB_E_SHAPE, "host_xcd_remap: bad argument");
    unsigned bx, by, bz;
    xcd_remap_calc((unsigned)gx, (unsigned)gy, (unsigned)gz, (unsigned)lin, bx, by, bz);
    xyz[0] = (int32_t)bx; xyz[1] = (int32_t)by; xyz[2] = (int32_t)bz;
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- glue + warp
extern "C" int vstab_flow_resize_scale(const float *flow, int B, int h, int w, float *out, int oh, int ow, int net_h, int net_w,
                                       void *stream)
{
    if (!flow || !out) return fail(nullptr, VSTAB_E_STATE, "flow_resize_scale: NULL buffer");
    if (B < 1 || h < 1 || w < 1 || oh < 1 || ow < 1 || net_h < 1 || net_w < 1) return fail(nullptr, VSTAB_E_SHAPE, "flow_resize_scale: bad shape");
    if (((uintptr_t)flow & 7) || ((uintptr_t)out & 7)) return fail(nullptr, VSTAB_E_ALIGN, "flow_resize_scale: 8-byte alignment");
    HIP_TRY(nullptr, launch_flow_resize_scale(flow, B, h, w, out, oh, ow, net_h, net_w, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_selftest_div_const(float d, unsigned first_bits, unsigned long long count, unsigned long long *bad_count_dev, void *stream)
{
    if (!bad_count_dev) return fail(nullptr, VSTAB_E_STATE, "selftest_div_const: NULL counter");
    if (count < 1 || count > (1ull << 32)) return fail(nullptr, VSTAB_E_SHAPE, "selftest_div_const: 1 <= count <= 2^32");
    const hipError_t e = launch_div_const_selftest(d, first_bits, count, bad_count_dev, (hipStream_t)stream);
    if (e == hipErrorInvalidValue) return fail(nullptr, VSTAB_E_SHAPE, "selftest_div_const: the glue takes the plain division for this divisor");
    HIP_TRY(nullptr, e);
    return VSTAB_OK;
}

extern "C" int vstab_resize_bilinear(const float *x, int B, int h, int w, int C, float *out, int oh, int ow, void *stream)
{
    if (!x || !out) return fail(nullptr, VSTAB_E_STATE, "resize_bilinear: NULL buffer");
    if (B < 1 || h < 1 || w < 1 || C < 1 || oh < 1 || ow < 1) return fail(nullptr, VSTAB_E_SHAPE, "resize_bilinear: bad shape");
    HIP_TRY(nullptr, launch_resize_bilinear(x, B, h, w, C, out, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_resize_bilinear_slice3(const float *x, int B, int h, int w, int Cs, int c_off, float *out, int oh, int ow, void *stream)
{
    if (!x || !out) return fail(nullptr, VSTAB_E_STATE, "resize_bilinear_slice3: NULL buffer");
    if (B < 1 || h < 1 || w < 1 || oh < 1 || ow < 1 || Cs < 3 || c_off < 0 || c_off + 3 > Cs)
        return fail(nullptr, VSTAB_E_SHAPE, "resize_bilinear_slice3: bad shape");
    if ((uintptr_t)out & 15) return fail(nullptr, VSTAB_E_ALIGN, "resize_bilinear_slice3: out must be 16-byte aligned");
    const hipError_t e = launch_resize_bilinear_slice3(x, B, h, w, Cs, c_off, out, oh, ow, (hipStream_t)stream);
    if (e == hipErrorNotSupported) return fail(nullptr, VSTAB_E_SHAPE, "resize_bilinear_slice3: problem too large");
    HIP_TRY(nullptr, e);
    return VSTAB_OK;
}

extern "C" int vstab_warp_flow(const float *img, const float *flow, float *out, int B, int H, int W, int C, void *stream)
{
    if (!img || !flow || !out) return fail(nullptr, VSTAB_E_STATE, "warp_flow: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 1) return fail(nullptr, VSTAB_E_SHAPE, "warp_flow: bad shape");
    if ((uintptr_t)flow & 7) return fail(nullptr, VSTAB_E_ALIGN, "warp_flow: flow must be 8-byte aligned");
    TraceRange range("tf_warp");
    HIP_TRY(nullptr, launch_warp_flow(img, flow, out, B, H, W, C, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_flow_glue_warp(const float *flow, int B, int h, int w, const float *img, float *outflow, float *warped, int oh,
                                    int ow, int C, int net_h, int net_w, void *stream)
{
    if (!flow || !img || !warped) return fail(nullptr, VSTAB_E_STATE, "flow_glue_warp: NULL buffer");
    if (B < 1 || h < 1 || w < 1 || oh < 1 || ow < 1 || net_h < 1 || net_w < 1) return fail(nullptr, VSTAB_E_SHAPE, "flow_glue_warp: bad shape");
    if (C != 3 || w < 2) return fail(nullptr, VSTAB_E_SHAPE, "flow_glue_warp: C must be 3 and w >= 2 (use flow_resize_scale + warp_flow otherwise)");
    if ((long long)B * oh * ow >= (1ll << 31)) return fail(nullptr, VSTAB_E_SHAPE, "flow_glue_warp: B*oh*ow must be < 2^31");
    if (((uintptr_t)flow & 7) || (((uintptr_t)img | (uintptr_t)outflow | (uintptr_t)warped) & 15))
        return fail(nullptr, VSTAB_E_ALIGN, "flow_glue_warp: flow 8-byte, img/outflow/warped 16-byte alignment");
    TraceRange range("flow_glue+tf_warp");
    HIP_TRY(nullptr, launch_flow_glue_warp(flow, B, h, w, img, outflow, warped, oh, ow, C, net_h, net_w, (hipStream_t)stream));
    return VSTAB_OK;
}

#if defined(VSTAB_HARNESS) && defined(VSTAB_STAMP)
// diagnostic build only (scripts/insitu_stamps.py): per-workgroup s_memtime stamps of the conv launches of a forward
namespace vstab { void conv_stamp_reset(); hipError_t conv_read_stamps_slot(int slot, unsigned long long *host, size_t n); }
extern "C" __attribute__((visibility("default"))) int vstab_debug_stamp_reset(void) { vstab::conv_stamp_reset(); return 0; }
extern "C" __attribute__((visibility("default"))) int vstab_debug_stamp_read(int slot, unsigned long long *host, size_t n)
{
    return vstab::conv_read_stamps_slot(slot, host, n) == hipSuccess ? 0 : -3;
}
#endif

extern "C" int vstab_hbm_profile_enable(int mode)
{
    if (mode < 0 || mode > 2) return fail(nullptr, VSTAB_E_SHAPE, "hbm_profile_enable: mode must be 0, 1 or 2");
    hbm_profile_enable(mode);
    return VSTAB_OK;
}

extern "C" int vstab_hbm_profile_read(int slot, double *ms_sum, int *launches, double *alg_bytes_sum)
{
    if (!ms_sum || !launches || !alg_bytes_sum) return fail(nullptr, VSTAB_E_STATE, "hbm_profile_read: NULL argument");
    if (slot < 0 || slot >= HBM_SLOTS) return fail(nullptr, VSTAB_E_SHAPE, "hbm_profile_read: slot out of range");
    HIP_TRY(nullptr, hbm_profile_read(slot, ms_sum, launches, alg_bytes_sum));
    return VSTAB_OK;
}

extern "C" int vstab_get_pixel_value(const float *img, const int32_t *x, const int32_t *y, float *out, int B, int H,
                                     int W, int C, int Hi, int Wi, void *stream)
{
    if (!img || !x || !y || !out) return fail(nullptr, VSTAB_E_STATE, "get_pixel_value: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || Hi < 1 || Wi < 1) return fail(nullptr, VSTAB_E_SHAPE, "get_pixel_value: bad shape");
    HIP_TRY(nullptr, launch_get_pixel_value(img, x, y, out, B, H, W, C, Hi, Wi, (hipStream_t)stream));
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- backward of tf_warp, get_pixel_value and the flow glue
extern "C" int vstab_warp_flow_backward(const float *img, const float *flow, const float *dout, int B, int H, int W, int C, float *d_img,
                                        float *d_flow, int accumulate_img, void *stream)
{
    if (!img || !flow || !dout) return fail(nullptr, VSTAB_E_STATE, "warp_flow_backward: NULL buffer");
    if (!d_img && !d_flow) return fail(nullptr, VSTAB_E_SHAPE, "warp_flow_backward: d_img and d_flow are both NULL");
    if (B < 1 || H < 1 || W < 1 || C < 1 || (long long)H * W >= (1ll << 31) || (long long)B * H * W >= (1ll << 39))
        return fail(nullptr, VSTAB_E_SHAPE, "warp_flow_backward: bad shape (H*W < 2^31, B*H*W < 2^39)");
    if (((uintptr_t)flow | (uintptr_t)d_flow) & 7) return fail(nullptr, VSTAB_E_ALIGN, "warp_flow_backward: flow and d_flow must be 8-byte aligned");
    TraceRange range("tf_warp backward");
    HIP_TRY(nullptr, launch_warp_flow_backward(img, flow, dout, B, H, W, C, d_img, d_flow, accumulate_img ? 1 : 0, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_get_pixel_value_backward(const float *dout, const int32_t *x, const int32_t *y, float *d_img, int B, int H, int W, int C,
                                              int Hi, int Wi, int accumulate, void *stream)
{
    if (!dout || !x || !y || !d_img) return fail(nullptr, VSTAB_E_STATE, "get_pixel_value_backward: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 1 || Hi < 1 || Wi < 1 || (long long)H * W >= (1ll << 31) || (long long)B * H * W >= (1ll << 39))
        return fail(nullptr, VSTAB_E_SHAPE, "get_pixel_value_backward: bad shape (H*W < 2^31, B*H*W < 2^39)");
    HIP_TRY(nullptr, launch_get_pixel_value_backward(dout, x, y, d_img, B, H, W, C, Hi, Wi, accumulate ? 1 : 0, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_flow_resize_scale_backward(const float *dout, int B, int oh, int ow, float *d_flow, int h, int w, int net_h, int net_w,
                                                void *stream)
{
    if (!dout || !d_flow) return fail(nullptr, VSTAB_E_STATE, "flow_resize_scale_backward: NULL buffer");
    if (B < 1 || B > 65535 || h < 1 || w < 1 || oh < 1 || ow < 1 || net_h < 1 || net_w < 1 || (long long)h * w * 2 >= (1ll << 31))
        return fail(nullptr, VSTAB_E_SHAPE, "flow_resize_scale_backward: bad shape (B <= 65535, h*w*2 < 2^31)");
    HIP_TRY(nullptr, launch_flow_resize_scale_backward(dout, B, oh, ow, d_flow, h, w, net_h, net_w, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_scale_shift(const float *x, long long npix, int C, float scale, const float *mean, float *out, void *stream)
{
    if (!x || !mean || !out) return fail(nullptr, VSTAB_E_STATE, "scale_shift: NULL buffer");
    if (npix < 1 || C < 1 || C > 4) return fail(nullptr, VSTAB_E_SHAPE, "scale_shift: bad shape");
    HIP_TRY(nullptr, launch_scale_shift(x, npix, C, scale, mean, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_maxpool2x2(const float *x, int B, int H, int W, int C, float *out, void *stream)
{
    if (!x || !out) return fail(nullptr, VSTAB_E_STATE, "maxpool2x2: NULL buffer");
    if (B < 1 || H < 1 || W < 1 || C < 4 || (C & 3)) return fail(nullptr, VSTAB_E_SHAPE, "maxpool2x2: bad shape (C must be a multiple of 4)");
    HIP_TRY(nullptr, launch_maxpool2x2(x, B, H, W, C, out, (hipStream_t)stream));
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- clip driver pieces
extern "C" int vstab_resize_u8(const uint8_t *src, int B, int sh, int sw, uint8_t *dst, int dh, int dw, void *stream)
{
    if (!src || !dst) return fail(nullptr, VSTAB_E_STATE, "resize_u8: NULL buffer");
    if (B < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1) return fail(nullptr, VSTAB_E_SHAPE, "resize_u8: bad shape");
    HIP_TRY(nullptr, launch_resize_u8(src, B, sh, sw, dst, dh, dw, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_resize_f32_to_u8(const float *src, int B, int sh, int sw, uint8_t *dst, int dh, int dw, void *stream)
{
    if (!src || !dst) return fail(nullptr, VSTAB_E_STATE, "resize_f32_to_u8: NULL buffer");
    if (B < 1 || sh < 1 || sw < 1 || dh < 1 || dw < 1) return fail(nullptr, VSTAB_E_SHAPE, "resize_f32_to_u8: bad shape");
    HIP_TRY(nullptr, launch_resize_f32_to_u8(src, B, sh, sw, dst, dh, dw, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_assemble_input(const uint8_t *const *slots9, int B, int h, int w, float *feats, void *stream)
{
    if (!slots9 || !feats) return fail(nullptr, VSTAB_E_STATE, "assemble_input: NULL buffer");
    for (int j = 0; j < 9; ++j)
        if (!slots9[j]) return fail(nullptr, VSTAB_E_STATE, "assemble_input: slot %d is NULL", j);
    if (B < 1 || h < 1 || w < 1) return fail(nullptr, VSTAB_E_SHAPE, "assemble_input: bad shape");
    if ((uintptr_t)feats & 15) return fail(nullptr, VSTAB_E_ALIGN, "assemble_input: feats must be 16-byte aligned");
    HIP_TRY(nullptr, launch_assemble_input(slots9, B, h, w, feats, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_assemble_input_resized(const uint8_t *const *slots8, const uint8_t *frame, int B, int h, int w, int sh, int sw, float *feats,
                                            void *stream)
{
    if (!slots8 || !frame || !feats) return fail(nullptr, VSTAB_E_STATE, "assemble_input_resized: NULL buffer");
    if (B < 1 || h < 1 || w < 1 || sh < 1 || sw < 1) return fail(nullptr, VSTAB_E_SHAPE, "assemble_input_resized: bad shape");
    if ((uintptr_t)feats & 15) return fail(nullptr, VSTAB_E_ALIGN, "assemble_input_resized: feats must be 16-byte aligned");
    HIP_TRY(nullptr, launch_assemble_input_resized(slots8, frame, B, h, w, sh, sw, feats, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_assemble_train_batch_launch_samples(void) { return TRAIN_BATCH_LAUNCH_SAMPLES; }

extern "C" int vstab_assemble_train_batch(const uint8_t *stab, const uint8_t *unstab, int N, int sh, int sw, const int *rows, const int *frame_idx, int n,
                                          float *feats, float *gtstab, float *unstab_out, int B, int H, int W, void *stream)
{
    if (!stab || !unstab || !rows || !frame_idx || !feats || !gtstab || !unstab_out)
        return fail(nullptr, VSTAB_E_STATE, "assemble_train_batch: NULL buffer");
    if (N < 1 || sh < 1 || sw < 1 || n < 1 || B < 1 || H < 1 || W < 1)
        return fail(nullptr, VSTAB_E_SHAPE, "assemble_train_batch: bad shape (N %d, source %dx%d, n %d, B %d, output %dx%d)", N, sh, sw, n, B, H, W);
    if ((long long)H * W > (1ll << 30) || (long long)sh * sw > (1ll << 30))
        return fail(nullptr, VSTAB_E_SHAPE, "assemble_train_batch: a frame of more than 2^30 pixels");
    if ((uintptr_t)feats & 15) return fail(nullptr, VSTAB_E_SHAPE, "assemble_train_batch: feats must be 16-byte aligned");
    if (((uintptr_t)gtstab | (uintptr_t)unstab_out) & 3) return fail(nullptr, VSTAB_E_SHAPE, "assemble_train_batch: gtstab / unstab_out must be 4-byte aligned");
    std::vector<char> seen((size_t)B, 0);
    for (int i = 0; i < n; ++i) {
        const int r = rows[i];
        if (r < 0 || r >= B) return fail(nullptr, VSTAB_E_SHAPE, "assemble_train_batch: rows[%d] = %d is outside [0, %d)", i, r, B);
        if (seen[(size_t)r]) return fail(nullptr, VSTAB_E_SHAPE, "assemble_train_batch: row %d is written twice (rows[%d])", r, i);
        seen[(size_t)r] = 1;
        for (int j = 0; j < 9; ++j) {
            const int f = frame_idx[(size_t)i * 9 + j];
            if (f < 0 || f >= N) return fail(nullptr, VSTAB_E_SHAPE, "assemble_train_batch: frame_idx[%d][%d] = %d is outside [0, %d)", i, j, f, N);
        }
    }
    TraceRange range("assemble_train_batch");
    HIP_TRY(nullptr, launch_assemble_train_batch(stab, unstab, sh, sw, rows, frame_idx, n, feats, gtstab, unstab_out, H, W, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_flow_glue_warp_u8(const float *flow, int B, int h, int w, const uint8_t *frame, float *outflow, uint8_t *out, int oh, int ow,
                                       int net_h, int net_w, void *stream)
{
    if (!flow || !frame || !out) return fail(nullptr, VSTAB_E_STATE, "flow_glue_warp_u8: NULL buffer");
    if (B < 1 || h < 1 || w < 2 || oh < 1 || ow < 1 || net_h < 1 || net_w < 1) return fail(nullptr, VSTAB_E_SHAPE, "flow_glue_warp_u8: bad shape (w >= 2)");
    if ((long long)B * oh * ow >= (1ll << 31) / 3) return fail(nullptr, VSTAB_E_SHAPE, "flow_glue_warp_u8: 3*B*oh*ow must be < 2^31");
    if (((uintptr_t)flow & 7) || ((uintptr_t)outflow & 7) || ((uintptr_t)out & 3))
        return fail(nullptr, VSTAB_E_ALIGN, "flow_glue_warp_u8: flow / outflow 8-byte, out 4-byte alignment");
    TraceRange range("frame_to_float+flow_glue+tf_warp+quantise");
    HIP_TRY(nullptr, launch_flow_glue_warp_u8(flow, B, h, w, frame, outflow, out, oh, ow, net_h, net_w, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_frame_to_float(const uint8_t *frame, long long npix, float *out, void *stream)
{
    if (!frame || !out || npix < 1) return fail(nullptr, VSTAB_E_STATE, "frame_to_float: bad argument");
    HIP_TRY(nullptr, launch_frame_to_float(frame, npix, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_quantise_output(const float *warped, long long npix, uint8_t *out, void *stream)
{
    if (!warped || !out || npix < 1) return fail(nullptr, VSTAB_E_STATE, "quantise_output: bad argument");
    HIP_TRY(nullptr, launch_quantise_output(warped, npix, out, (hipStream_t)stream));
    return VSTAB_OK;
}

// ------------------------------------------------------------------------- flow post-filters
extern "C" int vstab_flow_box_blur(const float *flow, int B, int h, int w, int k, float *tmp, float *out, void *stream)
{
    if (!flow || !tmp || !out) return fail(nullptr, VSTAB_E_STATE, "flow_box_blur: NULL buffer");
    if (B < 1 || h < 1 || w < 1 || k < 1 || !(k & 1)) return fail(nullptr, VSTAB_E_SHAPE, "flow_box_blur: bad shape (k must be odd)");
    HIP_TRY(nullptr, launch_flow_box_blur(flow, B, h, w, k, tmp, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_axpby(const float *x, float a, const float *y, float b, float *out, long long n, void *stream)
{
    if (!x || !y || !out || n < 1) return fail(nullptr, VSTAB_E_STATE, "axpby: bad argument");
    HIP_TRY(nullptr, launch_axpby(x, a, y, b, out, n, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_flow_medfilt(const float *flow, int B, int h, int w, int kh, int kw, int kc, float *out, void *stream)
{
    if (!flow || !out) return fail(nullptr, VSTAB_E_STATE, "flow_medfilt: NULL buffer");
    if (flow == out) return fail(nullptr, VSTAB_E_STATE, "flow_medfilt: in-place filtering is not supported");
    if (B < 1 || h < 1 || w < 1) return fail(nullptr, VSTAB_E_SHAPE, "flow_medfilt: bad shape");
    if (kh < 1 || kw < 1 || kc < 1 || !(kh & 1) || !(kw & 1) || !(kc & 1) || kh > 31 || kw > 31 || kc > 5)
        return fail(nullptr, VSTAB_E_SHAPE, "flow_medfilt: kernel sizes must be odd, kh,kw <= 31, kc <= 5");
    HIP_TRY(nullptr, launch_flow_medfilt(flow, B, h, w, kh, kw, kc, out, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" size_t vstab_homography_workspace_bytes(int B, int H, int W, int K)
{
    if (B < 1 || H < 1 || W < 1 || K < 1 || K > 512) return 0;
    return homography_workspace_bytes(B, H, W, K);
}

extern "C" int vstab_homography_fit(const float *flow, int B, int H, int W, int K, unsigned seed, double thresh, int refine,
                                    int stride, double *Hout, int32_t *inliers, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    if (!flow || !Hout || !inliers || !workspace) return fail(nullptr, VSTAB_E_STATE, "homography_fit: NULL buffer");
    if (B < 1 || H < 2 || W < 2 || (long long)H * W > 0x7fffffffLL) return fail(nullptr, VSTAB_E_SHAPE, "homography_fit: bad shape");
    if (K < 1 || K > 512 || refine < 1 || refine > 16 || stride < 1 || !(thresh > 0.0))
        return fail(nullptr, VSTAB_E_SHAPE, "homography_fit: need 1 <= K <= 512, 1 <= refine <= 16, stride >= 1, thresh > 0");
    if (workspace_bytes < homography_workspace_bytes(B, H, W, K)) return fail(nullptr, VSTAB_E_NOMEM, "homography_fit: workspace too small");
    if (((uintptr_t)flow | (uintptr_t)Hout | (uintptr_t)workspace) & 7)
        return fail(nullptr, VSTAB_E_ALIGN, "homography_fit: flow / Hout / workspace must be 8-byte aligned");
    HIP_TRY(nullptr, launch_homography_fit(flow, B, H, W, K, seed, thresh, refine, stride, Hout, inliers, workspace, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_warp_perspective_u8(const uint8_t *src, int B, int sh, int sw, const double *Hm, uint8_t *dst, int oh, int ow,
                                         void *stream)
{
    if (!src || !Hm || !dst) return fail(nullptr, VSTAB_E_STATE, "warp_perspective_u8: NULL buffer");
    if (src == dst) return fail(nullptr, VSTAB_E_STATE, "warp_perspective_u8: in-place warping is not supported");
    if (B < 1 || sh < 1 || sw < 1 || oh < 1 || ow < 1 || sh > 32767 || sw > 32767)
        return fail(nullptr, VSTAB_E_SHAPE, "warp_perspective_u8: bad shape");
    HIP_TRY(nullptr, launch_warp_perspective_u8(src, B, sh, sw, Hm, dst, oh, ow, (hipStream_t)stream));
    return VSTAB_OK;
}

extern "C" int vstab_flow_mean_fill(const float *flow, int B, int h, int w, float *out, void *stream)
{
    if (!flow || !out) return fail(nullptr, VSTAB_E_STATE, "flow_mean_fill: NULL buffer");
    if (B < 1 || h < 1 || w < 1) return fail(nullptr, VSTAB_E_SHAPE, "flow_mean_fill: bad shape");
    HIP_TRY(nullptr, launch_flow_mean_fill(flow, B, h, w, out, (hipStream_t)stream));
    return VSTAB_OK;
}
